function [X,it,rel_res,rel_resk,rhok] = Class_AMG_multi(varargin)
% [X,it,rel_res,rel_resk,rhok] = Class_AMG_multi(A,B,amg_options): one Class_AMG setup, then every
% column of B through its solve phase as if solved alone (X(:,j), it(j), rel_res(j); column j of
% rel_resk / rhok holds its history, NaN past it(j)+1).  Leaves the hierarchy for MG_Vcycle /
% MG_Wcycle as Class_AMG does.  Forwards to libipdamg (HIP, gfx950) through the MEX gateway ipd_mex.
% See INTEGRATION.md.
[X,it,rel_res,rel_resk,rhok] = ipd_mex('Class_AMG_multi', varargin{:});
end
