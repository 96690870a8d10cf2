function [H,info] = nmf_inf_fp(A,W,H,vary,varargin)
% NMF_INF_FP - fixed-point inference of the NMF activations H with W held fixed, ON THE GPU
%
% [H,info] = nmf_inf_fp(A,W,H,vary [,opts])
% The argument list of experiments/nmf/nmf_inf_fp.m: A T x D (>= 0), W K x D, H T x K (> 0), vary T x D, a scalar or [] (= zeros),
% opts.numIts (default 100).  The iterations run in libnagp.so (nagp_nmf_fp with update_w = 0, include/nagp.h); this file only
% marshals arguments.  info.Obj holds one objective per iteration.
% As in the reference, W is normalised only when EVERY row sum differs from 1 (an `if` on a vector); a W with one row sum exactly 1
% goes through as it is.

  numIts = 100;
  if nargin > 4 && isfield(varargin{1}, 'numIts'), numIts = varargin{1}.numIts; end
  if isscalar(vary), vary = vary * ones(size(A)); end
  rs = sum(W, 2);
  if all(rs ~= 1), W = bsxfun(@times, 1 ./ rs, W); end
  [~, H, Obj] = nagp_mex('nmf_fp', A, vary, W, H, numIts, 0);
  info.Obj = Obj(:)';
end
