function [Obj,varargout] = get_Obj_pSTFT_all(theta,vary,specTar,minVar,limOm,limLam,bet,kernel)
% GET_OBJ_PSTFT_ALL - objective (and gradient) of the filterbank spectrum fit for any served kernel, ON THE GPU
%
% [Obj,dObj] = get_Obj_pSTFT_all(theta,vary,specTar,minVar,limOm,limLam,bet,kernel)
% The argument list of unifying_prob_tf/get_Obj_pSTFT_all.m; kernel 'exp', 'matern32', 'matern52' or 'matern72' ('se' is refused, as
% everywhere in this library).  The file's quirk is kept: len = sqrt(5) / lam for every kernel except exp and matern32, so matern72
% runs with sqrt(5).  Put ahead of the reference's file on the path, it lets the reference's fit_probSTFT_SD.m and minimize.m run
% unchanged on the device objective (nagp_pstft_obj, include/nagp.h).  dObj is formed only when asked for.

  if nargout > 1
    [Obj, dObj] = nagp_mex('pstft_obj', kernel, 1, theta(:), vary, specTar(:), minVar(:), limOm, limLam, bet);
    varargout{1} = dObj;
  else
    Obj = nagp_mex('pstft_obj', kernel, 1, theta(:), vary, specTar(:), minVar(:), limOm, limLam, bet);
  end
end
