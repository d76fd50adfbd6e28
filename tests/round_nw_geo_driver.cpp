// CPU driver of the north-west correction's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_round_nw_geo.h) for tests/test_round_nw_geo.py.  One query per input
// line, `<what> <m> <n>`:
//   geo     the chunks of the two scans, the buffer sizes and the bytes a side and the workspace take
//   reach   walks every index k_nw_scan writes into the prefixes and the dense slots, every prefix a breakpoint
//           thread of k_nw_merge may read, the slot of every (k, s), and the slots k_nw_last's threads own
// Per query it prints one line:
//   geo chm= chn= pre= slots= span= cap= scratch= workspace=
//   reach pw=<largest prefix written> pr=<largest read> punwritten= pdup= plen= sw=<largest slot marked> sdup= slen=
//         slotmin= slotmax= owned=<slots owned by a thread> owndup= chunkmax=<largest chunk a scan thread has> outside=
// The first line of the output is
//   limits NW_CHUNK= NW_THREADS= NW_MAX_LEN= NW_INFO_DOUBLES= NW_DEV_DOUBLES=
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "geo_buf.h"
#include "ipd_round_nw_geo.h"

int main() {
    std::printf("limits NW_CHUNK=%d NW_THREADS=%d NW_MAX_LEN=%d NW_INFO_DOUBLES=%d NW_DEV_DOUBLES=%d\n", NW_CHUNK,
                NW_THREADS, NW_MAX_LEN, NW_INFO_DOUBLES, NW_DEV_DOUBLES);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0;
        if (!(in >> what >> m >> n) || m < 1 || n < 1) continue;
        const int slots = nw_slots(m, n);
        if (what == "geo") {
            std::printf("geo chm=%d chn=%d pre=%zu slots=%d span=%d cap=%zu scratch=%zu workspace=%zu\n", nw_chunks(m),
                        nw_chunks(n), nw_pre_len(m, n), slots, nw_span(slots), nw_list_cap(m, n),
                        round_nw_scratch_bytes(m, n), round_nw_workspace_bytes(m, n));
        } else if (what == "reach") {
            Buf pre(nw_pre_len(m, n)), slot(nw_list_cap(m, n)), own((size_t)slots);
            int chunkmax = 0;
            // k_nw_scan: workgroup 0 the columns, 1 the rows; entry 0 and one prefix per entry, thread c its chunk
            for (int blk = 0; blk < 2; ++blk) {
                const int len = blk == 0 ? n : m;
                const size_t base = blk == 0 ? nw_pre_col(0) : nw_pre_row(n, 0);
                pre.write(base);
                for (int c = 0; c < nw_chunks(len); ++c) {
                    chunkmax = std::max(chunkmax, c);
                    for (int k = c * NW_CHUNK; k < std::min(c * NW_CHUNK + NW_CHUNK, len); ++k) pre.write(base + 1 + (size_t)k);
                }
                for (int tid = 0; tid < NW_THREADS; ++tid)   // the dense slots marked empty
                    for (int k = blk * NW_THREADS + tid; k < slots; k += 2 * NW_THREADS) slot.write((size_t)k);
            }
            // k_nw_merge: a breakpoint thread reads its own prefix, the one before it, and any of the other vector
            for (int s = 0; s <= n; ++s) pre.read(nw_pre_col(s));
            for (int k = 0; k <= m; ++k) pre.read(nw_pre_row(n, k));
            int slotmin = slots, slotmax = -1;
            for (int k = 1; k <= m; k += std::max(1, m / 97))
                for (int s = 1; s <= n; s += std::max(1, n / 89)) {
                    slotmin = std::min(slotmin, nw_slot(k, s));
                    slotmax = std::max(slotmax, nw_slot(k, s));
                }
            slotmin = std::min(slotmin, nw_slot(1, 1));
            slotmax = std::max(slotmax, nw_slot(m, n));
            // k_nw_last: thread t owns [t*span, (t+1)*span) below the slot count
            const int span = nw_span(slots);
            for (int t = 0; t < NW_THREADS; ++t) {
                const int s0 = std::min(t * span, slots), s1 = std::min(s0 + span, slots);
                for (int k = s0; k < s1; ++k) {
                    own.write((size_t)k);
                    slot.read((size_t)k);
                }
            }
            size_t owned = 0;
            for (unsigned char w : own.written) owned += w;
            std::printf("reach pw=%zu pr=%zu punwritten=%zu pdup=%zu plen=%zu sw=%zu sdup=%zu slen=%zu slotmin=%d "
                        "slotmax=%d owned=%zu owndup=%zu chunkmax=%d outside=%d\n",
                        pre.wmax, pre.rmax, pre.unwritten, pre.dup, pre.len(), slot.wmax, slot.dup + slot.unwritten,
                        slot.len(), slotmin, slotmax, owned, own.dup, chunkmax,
                        (pre.outside || slot.outside || own.outside) ? 1 : 0);
        }
    }
    return 0;
}
