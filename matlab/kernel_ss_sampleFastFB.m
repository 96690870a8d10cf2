function [Ydraw,Xdraw,Xmean] = kernel_ss_sampleFastFB(A,Q,C,P0,K,vary,y,n_draws,varargin)
% KERNEL_SS_SAMPLEFASTFB - joint posterior draws of the stationary filterbank ON THE GPU (simulation smoother)
%
% [Ydraw,Xdraw,Xmean] = kernel_ss_sampleFastFB(A,Q,C,P0,K,vary,y,n_draws [,seed [,Lq [,Lp]]])
% Same model arguments as kernel_ss_kalmanFastFB (P0 = Pinf, NaN in y = missing) and the same set-up lines (dare, stationary
% gain, smoother gain).  Draw i:  x* from the prior (x*_0 = Lp*z_0, x*_t = A*x*_{t-1} + Lq*z_t), y* = C*x* + sqrt(vary)*e where
% y is observed, X_i = x* + S_y(y - y*), Ydraw(:,i) = C*X_i, with S_y(.) the smoothed means of kernel_ss_kalmanFastFB and z, e
% from the counter-based generator of libnagp.so keyed by seed (nagp_fastfb_sample, include/nagp.h).  Whole trajectories,
% correlated in time: the mean over draws is S_y(y) in expectation, the covariance is the error covariance of the steady-state
% smoother under the model -- Psm away from the ends and from gaps, larger inside gaps.
% Ydraw is T x n_draws, Xdraw S x T x n_draws (computed only when asked for), Xmean = S_y(y) is S x T.
% Lq, Lp: factors with Lq*Lq' = Q, Lp*Lp' = P0 (default: chol(.,'lower'); symmetric eigen-factor with negative eigenvalues
% clipped to 0 when that fails).

  if nargin <= 8 || isempty(varargin{1}), seed = 0; else, seed = varargin{1}; end
  if nargin <= 9 || isempty(varargin{2}), Lq = lower_factor(Q); else, Lq = varargin{2}; end
  if nargin <= 10 || isempty(varargin{3}), Lp = lower_factor(P0); else, Lp = varargin{3}; end
  H = C; R = vary;
  try
    PP = dare(A',H',Q,R);
    S = H*PP*H' + R;
  catch
    error('Unstable DARE solution!')
  end
  Kg = PP*H'/S;
  AKHA = A - Kg*H*A;
  PF2 = PP - Kg*H*PP;
  HA = H*A;
  G = PF2*A'/PP;
  if nargout > 2
    [Ydraw,Xdraw,Xmean] = nagp_mex('fastfb_sample', A, AKHA, HA(:), Kg(:), G, H(:), R, Lp, Lq, y(:), n_draws, seed);
  elseif nargout > 1
    [Ydraw,Xdraw] = nagp_mex('fastfb_sample', A, AKHA, HA(:), Kg(:), G, H(:), R, Lp, Lq, y(:), n_draws, seed);
  else
    Ydraw = nagp_mex('fastfb_sample', A, AKHA, HA(:), Kg(:), G, H(:), R, Lp, Lq, y(:), n_draws, seed);
  end
end

function F = lower_factor(P)
  P = (P+P')/2;
  [F,flag] = chol(P,'lower');
  if flag ~= 0
    [V,E] = eig(P);
    F = V*diag(sqrt(max(diag(E),0)));
  end
end
