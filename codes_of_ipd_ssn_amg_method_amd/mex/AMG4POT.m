function [zeta,itamg,resamg,info] = AMG4POT(prob_data,amg_options,str)
% Drop-in shim (Class2/AMG4POT.m:1): str = 'amg' (Hybrid_AMG) or 'twogrid' (Hybrid_twogrid); new:
% 'amg_pcg' (Hybrid_AMG_PCG: AMG-preconditioned CG as the inner solver of both solves).
if strcmp(str,'amg')
    [zeta,itamg,resamg,info] = ipd_mex('AMG4POT', prob_data, amg_options);
elseif strcmp(str,'amg_pcg')
    [zeta,itamg,resamg,info] = ipd_mex('AMG4POT_pcg', prob_data, amg_options);
else
    [zeta,itamg,resamg,info] = ipd_mex('AMG4POT_twogrid', prob_data, amg_options);
end
end
