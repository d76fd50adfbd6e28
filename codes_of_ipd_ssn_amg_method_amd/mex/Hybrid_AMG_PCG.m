function [zeta,itamg,resamg,info] = Hybrid_AMG_PCG(prob_data,amg_options)
% [zeta,itamg,resamg,info] = Hybrid_AMG_PCG(prob_data,amg_options): Hybrid_AMG.m with every Class_AMG
% call replaced by its setup followed by AMG-preconditioned CG (AMG_PCG) from the same random guess:
% same rescaling, components, isnsp / fnode rule, rand stream and small-block direct solves.  retol and
% maxit are amg_options'; itamg / resamg are the largest PCG count / res over the large components.
% Forwards to libipdamg (HIP, gfx950) through the MEX gateway ipd_mex.  See INTEGRATION.md.
[zeta,itamg,resamg,info] = ipd_mex('Hybrid_AMG_PCG', prob_data, amg_options);
end
