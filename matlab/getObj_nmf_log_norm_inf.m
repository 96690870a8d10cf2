function [obj,dobj] = getObj_nmf_log_norm_inf(x,A,W,vary,lenx,mux,varx,tol)
% GETOBJ_NMF_LOG_NORM_INF - objective (and gradient) of temporal NMF inference with exp(squared-exponential GP) activations and a fixed W, ON THE GPU
%
% [obj,dobj] = getObj_nmf_log_norm_inf(x,A,W,vary,lenx,mux,varx,tol)
% The argument list of experiments/nmf/getObj_nmf_log_norm_inf.m: x [T*K,1] = X(:), A [T,D] data, W [K,D] spectral basis (used as given, not
% renormalised), vary [T,D] observation noise ([] = zeros), lenx, mux, varx [1,K], tol the extent of the basis functions.  Put ahead of the
% reference's file on the path, it lets the reference's tnmf_inf.m and minimize.m run unchanged on the device objective (nagp_tnmf_obj).

  out = cell(1, max(nargout, 1));                     % nlhs of the gateway = nargout: dobj is formed only when asked for
  [out{:}] = nagp_mex('tnmf_obj', x(:), A, vary, W, lenx, mux, varx, tol);
  obj = out{1};
  if nargout > 1
    dobj = out{2};
  end
end
