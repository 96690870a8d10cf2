function [obj,dobj] = getObj_nmf_log_norm(xlogW,A,vary,lenx,mux,varx,tol)
% GETOBJ_NMF_LOG_NORM - objective (and gradient) of temporal NMF with exp(squared-exponential GP) activations, ON THE GPU
%
% [obj,dobj] = getObj_nmf_log_norm(xlogW,A,vary,lenx,mux,varx,tol)
% The argument list of experiments/nmf/getObj_nmf_log_norm.m: xlogW [T*K+K*D,1] = [X(:); log(W(:))], A [T,D] data, vary [T,D] observation
% noise ([] = zeros), lenx, mux, varx [1,K], tol the extent of the basis functions.  Put ahead of the reference's file on the path, it lets
% the reference's tnmf.m and minimize.m run unchanged on the device objective (nagp_tnmf_obj, include/nagp.h).

  out = cell(1, max(nargout, 1));                     % nlhs of the gateway = nargout: dobj is formed only when asked for
  [out{:}] = nagp_mex('tnmf_obj', xlogW(:), A, vary, [], lenx, mux, varx, tol);
  obj = out{1};
  if nargout > 1
    dobj = out{2};
  end
end
