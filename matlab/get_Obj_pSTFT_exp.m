function [Obj,varargout] = get_Obj_pSTFT_exp(theta,vary,specTar,minVar,limOm,limLam,bet,dummy)
% GET_OBJ_PSTFT_EXP - objective (and gradient) of the filterbank spectrum fit for the exp kernel, ON THE GPU
%
% [Obj,dObj] = get_Obj_pSTFT_exp(theta,vary,specTar,minVar,limOm,limLam,bet [,dummy])
% The argument list of unifying_prob_tf/get_Obj_pSTFT_exp.m: theta 3D x 1, specTar N x 1, minVar D x 1, limOm, limLam D x 2.
% Put ahead of the reference's file on the path, it lets the reference's fit_probSTFT_SD.m and minimize.m run unchanged on the
% device objective (nagp_pstft_obj, include/nagp.h).  dObj is formed only when asked for.

  if nargout > 1
    [Obj, dObj] = nagp_mex('pstft_obj', 'exp', 0, theta(:), vary, specTar(:), minVar(:), limOm, limLam, bet);
    varargout{1} = dObj;
  else
    Obj = nagp_mex('pstft_obj', 'exp', 0, theta(:), vary, specTar(:), minVar(:), limOm, limLam, bet);
  end
end
