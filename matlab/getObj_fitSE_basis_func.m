function [obj,dobj] = getObj_fitSE_basis_func(z,x,lenx,varx,tol)
% GETOBJ_FITSE_BASIS_FUNC - objective (and gradient) of the basis-function fit of a squared-exponential GP to a signal, ON THE GPU
%
% [obj,dobj] = getObj_fitSE_basis_func(z,x,lenx,varx,tol)
% The argument list of experiments/toolsGP/getObj_fitSE_basis_func.m: z [T,1] basis-function coefficients, x [T,1] the signal, lenx, varx
% scalars, tol the extent of the basis functions.  Put ahead of the reference's file on the path, it lets the reference's fitSEGP_BF.m and
% minimize.m run unchanged on the device objective (nagp_sebf_fit_obj, include/nagp.h).

  out = cell(1, max(nargout, 1));                     % nlhs of the gateway = nargout: dobj is formed only when asked for
  [out{:}] = nagp_mex('sebf_fit_obj', z(:), x(:), lenx, varx, tol);
  obj = out{1};
  if nargout > 1
    dobj = out{2};
  end
end
