function [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary,varargin)
% GETOBJ_NMF_TEMP_INF - objective (and gradient) of NMF inference with temporal priors and a fixed W, ON THE GPU
%
% [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary)                       no temporal prior
% [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary,varinf,lam)            truncated-Gaussian chain
% [obj,dobj] = getObj_nmf_temp_inf(logH,A,W,vary,muinf,varinf,lam)      inverse-gamma Markov chain
% The argument list of experiments/nmf/getObj_nmf_temp_inf.m: logH [T*K,1], A [T,D] data, W [K,D] spectral basis (used as given, not
% renormalised), vary [T,D] observation noise, muinf, varinf, lam [1,K].  Put ahead of the reference's file on the path, it lets the
% reference's nmf_inf.m and minimize.m run unchanged on the device objective (nagp_nmf_temp_obj, include/nagp.h).

  if numel(varargin) == 1 || numel(varargin) > 3
    error('nagp:arg', 'no prior argument, (varinf,lam) or (muinf,varinf,lam)');
  end
  p = [cell(1, 3 - numel(varargin)), varargin];       % {muinf, varinf, lam}, [] where not given
  out = cell(1, max(nargout, 1));                     % nlhs of the gateway = nargout: dobj is formed only when asked for
  [out{:}] = nagp_mex('nmf_temp_obj', logH(:), A, vary, W, p{1}, p{2}, p{3});
  obj = out{1};
  if nargout > 1
    dobj = out{2};
  end
end
