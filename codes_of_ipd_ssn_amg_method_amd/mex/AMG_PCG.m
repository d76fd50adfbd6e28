function [d,it,res,resk] = AMG_PCG(varargin)
% [d,it,res,resk] = AMG_PCG(A,b,amg_options,pcg_options[,planned]): Class_AMG's hierarchy as the
% preconditioner of PCG.m's loop (one cycle per iteration, flexible beta).  planned (optional, default
% false): run the whole loop as ONE single-workgroup launch where the hierarchy is small enough for it
% (every level <= 1024 rows) and pcg_options.maxit <= 1000; the same launches otherwise.  Forwards to
% libipdamg (HIP, gfx950) through the MEX gateway ipd_mex.  See INTEGRATION.md.
[d,it,res,resk] = ipd_mex('AMG_PCG', varargin{:});
end
