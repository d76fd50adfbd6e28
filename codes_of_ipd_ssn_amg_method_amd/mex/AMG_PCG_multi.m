function [D,it,res,resk] = AMG_PCG_multi(varargin)
% [D,it,res,resk] = AMG_PCG_multi(A,B,amg_options,pcg_options): one Class_AMG setup, then every column
% of B through AMG_PCG's loop as if solved alone (D(:,j), it(j), res(j); column j of resk holds its
% history, NaN past it(j)).  A guess in pcg_options is size(B).  Forwards to libipdamg (HIP, gfx950)
% through the MEX gateway ipd_mex.  See INTEGRATION.md.
[D,it,res,resk] = ipd_mex('AMG_PCG_multi', varargin{:});
end
