function [lik,Xfin,Pfin,varargout] = kernel_ss_kalmanSlowFB(A,Q,C,P0,K,vary,y,varargin)
% KERNEL_SS_KALMANSLOWFB - exact Kalman filter / RTS smoother of the stationary filterbank ON THE GPU
%
% [lik,Xfin,Pfin] = kernel_ss_kalmanSlowFB(A,Q,C,P0,K,vary,y [,verbose [,KF [,cov [,sub_idx]]]])
% The argument list of unifying_prob_tf/kernel_ss_kalmanSlowFB_rewrite.m: time-varying covariance, vary a scalar or one
% observation variance per step.  The whole recursion runs in libnagp.so (nagp_slowfb_run, include/nagp.h); this file only
% marshals arguments.  NaN in y = missing (skips the update and the likelihood term of that step).
% Xfin is 1 x S x T.  Pfin by cov: 'full' (default) S x S x T, 'diag' S x T marginal variances, 'sub' the rows and columns
% sub_idx (1-based, ascending), 'none' [].  KF = 1 returns the filtered moments.
% A and Q must be block diagonal with blocks of at most 8 states (get_disc_model builds blocks of 2*tau).
% The EM sufficient statistics of the older kernel_ss_kalmanSlowFB.m (a fourth output) are not built.

  if nargout > 3
    error('nagp:unsupported', 'kernel_ss_kalmanSlowFB: the EM sufficient statistics (Ptsum, YX, A1-A3: lag-one covariances) are not built');
  end
  if nargin <= 8 || isempty(varargin{2}), KF = 0; else, KF = varargin{2}; end
  if nargin <= 9 || isempty(varargin{3}), cov = 'full'; else, cov = varargin{3}; end
  S = size(A,1); T = numel(y);
  if numel(vary) == 1, vary = vary*ones(T,1); end
  nz = (A ~= 0) | (Q ~= 0);
  block = S;
  for b = 1:min(8,S)
    if mod(S,b) == 0 && ~any(any(nz & ~kron(eye(S/b), ones(b))))
      block = b; break
    end
  end
  switch cov
    case 'full', code = 2; sub = int32(0:S-1);
    case 'sub',  code = 2; sub = int32(varargin{4}(:)' - 1);
    case 'diag', code = 1; sub = int32([]);
    otherwise,   code = 0; sub = int32([]);
  end
  if nargout > 2
    [lik,MS,Pfin] = nagp_mex('slowfb', A, Q, C(:), P0, block, y(:), vary(:), KF == 1, code, sub);
  else
    [lik,MS] = nagp_mex('slowfb', A, Q, C(:), P0, block, y(:), vary(:), KF == 1, code, sub);
  end
  Xfin = reshape(MS, [1 S T]);
end
