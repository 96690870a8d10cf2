function [Z,varargout] = kernel_ss_probFB(y,A,Q,C,P0,K,vary,tau,varargin)
% KERNEL_SS_PROBFB - probabilistic filterbank: complex sub-bands of y from the state-space smoother ON THE GPU
%
% [Z,covZ,Zfull,covZfull] = kernel_ss_probFB(y,A,Q,C,P0,K,vary,tau [,verbose [,KF [,slow]]])
% The argument list of unifying_prob_tf/kernel_ss_probFB.m.  slow = 0 (default): the steady-state smoother kernel_ss_kalmanFastFB;
% slow = 1: the exact smoother kernel_ss_kalmanSlowFB with an observation variance per step.  KF = 1: filtered moments.
% Z D x T complex; covZ 2D x 2D x T; Zfull, covZfull with the higher-order terms (getFBLDSOutput_tau).
% With slow = 1 only what the outputs need is asked of the smoother: no covariance for Z alone, the 2D rows of covZ ('sub') for two
% or three outputs, the full covariance only for covZfull.

  if nargin > 8,  verbose = varargin{1}; else, verbose = 0; end
  if nargin > 9,  KF = varargin{2};      else, KF = 0;      end
  if nargin > 10, slow = varargin{3};    else, slow = 0;    end
  varargout = cell(1, nargout - 1);
  if slow == 1 && nargout <= 1
    [~, Xfin] = kernel_ss_kalmanSlowFB(A, Q, C, P0, K, vary, y, verbose, KF, 'none');
    Z = getFBLDSOutput_tau(Xfin, [], tau);
  elseif slow == 1 && nargout <= 3
    S = size(A, 1);
    rows = sort([1:2*tau:S-1, 2:2*tau:S]);
    [~, Xfin, Psub] = kernel_ss_kalmanSlowFB(A, Q, C, P0, K, vary, y, verbose, KF, 'sub', rows);
    [~, re] = ismember(1:2*tau:S-1, rows); [~, im] = ismember(2:2*tau:S, rows);
    if nargout > 2
      [Z, ~, varargout{2}] = getFBLDSOutput_tau(Xfin, zeros(S, S, 0), tau);
    else
      Z = getFBLDSOutput_tau(Xfin, [], tau);
    end
    varargout{1} = Psub([re, im], [re, im], :);
  else
    if slow == 1
      [~, Xfin, Pfin] = kernel_ss_kalmanSlowFB(A, Q, C, P0, K, vary, y, verbose, KF);
    else
      [~, Xfin, Pfin] = kernel_ss_kalmanFastFB(A, Q, C, P0, K, vary, y, verbose, KF);
    end
    [Z, varargout{:}] = getFBLDSOutput_tau(Xfin, Pfin, tau);
  end
end
