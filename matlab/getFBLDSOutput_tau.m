function [S,varargout] = getFBLDSOutput_tau(Xfin,Pfin,tau)
% GETFBLDSOUTPUT_TAU - complex sub-bands and their covariances from the states of the filterbank smoother
%
% [S,covS,Sfull,covSfull] = getFBLDSOutput_tau(Xfin,Pfin,tau)
% The argument list of unifying_prob_tf/getFBLDSOutput_tau.m.  Xfin 1 x 2*D*tau x T, Pfin 2*D*tau x 2*D*tau x T; the state holds
% (real, imaginary) pairs, tau pairs per sub-band.  S D x T: the first pair of every sub-band as a complex number; covS 2D x 2D x T in
% [real; imaginary] order; Sfull and covSfull: the same for every pair.  Selection and pairing only -- nothing is computed.

  n2 = size(Xfin, 2);
  X = reshape(Xfin(1,:,:), n2, []);
  re1 = 1:2*tau:n2-1; im1 = re1 + 1;
  if nargout > 2
    Sfull = X(1:2:n2-1, :) + 1i * X(2:2:n2, :);
    S = Sfull(1:tau:end, :);
    varargout{2} = Sfull;
  else
    S = X(re1, :) + 1i * X(im1, :);
  end
  if nargout > 1
    sel = [re1, im1];
    varargout{1} = Pfin(sel, sel, :);
  end
  if nargout > 3
    sel = [1:2:n2-1, 2:2:n2];
    varargout{3} = Pfin(sel, sel, :);
  end
end
