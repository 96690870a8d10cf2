function [W,H,info] = nmf_fp(A,W,H,vary,varargin)
% NMF_FP - fixed-point NMF (A ~ H*W, rows of W summing to 1) ON THE GPU
%
% [W,H,info] = nmf_fp(A,W,H,vary [,opts])
% The argument list of experiments/nmf/nmf_fp.m: A T x D (>= 0), W K x D, H T x K (> 0), vary T x D, a scalar or [] (= zeros),
% opts.numIts (default 1000), opts.restarts.  The iterations run in libnagp.so (nagp_nmf_fp, include/nagp.h); this file marshals
% arguments, draws the restart candidates and picks among them.  info.Obj holds two objectives per iteration.
% With opts.restarts = R the first candidate is the caller's (W,H); the others are rows of A and exp(randn), drawn with MATLAB's own
% rand / randn in the reference's order (one draw of ks, then of H, after every candidate), so a MATLAB caller keeps the
% reference's random stream.  All R candidates run their 10 inference iterations as ONE batched gateway call; the smallest final
% objective wins, the earliest on a tie.  info.restart is the winner's index.

  numIts = 1000;
  if nargin > 4 && isfield(varargin{1}, 'numIts'), numIts = varargin{1}.numIts; end
  if isscalar(vary), vary = vary * ones(size(A)); end
  [T, K] = size(H); D = size(W, 2);
  if nargin > 4 && isfield(varargin{1}, 'restarts')
    R = varargin{1}.restarts;
    Wc = zeros(K, D, R); Wb = Wc; Hc = zeros(T, K, R);
    for r = 1:R
      Wc(:,:,r) = bsxfun(@times, 1 ./ sum(W, 2), W); Hc(:,:,r) = H;
      Wi = Wc(:,:,r); rs = sum(Wi, 2);
      if all(rs ~= 1), Wi = bsxfun(@times, 1 ./ rs, Wi); end      % what nmf_inf_fp does to its copy
      Wb(:,:,r) = Wi;
      ks = ceil(T * rand(K, 1)); W = A(ks, :); H = exp(randn(T, K));
    end
    [~, Hr, Obj] = nagp_mex('nmf_fp', A, vary, Wb, Hc, 10, 0);
    best = inf;
    for r = 1:R
      if Obj(end, r) < best, best = Obj(end, r); info.restart = r; end
    end
    W = Wc(:,:,info.restart); H = Hr(:,:,info.restart);
  end
  W = bsxfun(@times, 1 ./ sum(W, 2), W);
  [W, H, Obj] = nagp_mex('nmf_fp', A, vary, W, H, numIts, 1);
  info.Obj = Obj(:)';
end
