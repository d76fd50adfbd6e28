function [d,it,res,resk] = AMG_PCG(varargin)
% [d,it,res,resk] = AMG_PCG(A,b,amg_options,pcg_options): Class_AMG's hierarchy as the
% preconditioner of PCG.m's loop (one cycle per iteration, flexible beta).  Forwards to
% libipdamg (HIP, gfx950) through the MEX gateway ipd_mex.  See INTEGRATION.md.
[d,it,res,resk] = ipd_mex('AMG_PCG', varargin{:});
end
