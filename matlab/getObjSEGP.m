function [obj,dobj] = getObjSEGP(param,specy,varargin)
% GETOBJSEGP - negative log-likelihood (and gradient) of a regularly sampled squared-exponential GP in the spectral domain, ON THE GPU
%
% [obj,dobj] = getObjSEGP(param,specy)             param = [log(len); log(varx); log(vary)]
% [obj,dobj] = getObjSEGP(param,specy,vary)        param = [log(len); log(varx)]
% [obj,dobj] = getObjSEGP(param,specy,vary,varx)   param(1) = log(len)
% The argument list of experiments/toolsGP/getObjSEGP.m; specy = abs(fft(y)).^2.  Put ahead of the reference's file on the path, it
% lets the reference's trainSEGP_RS.m and minimize.m run unchanged on the device objective (nagp_segp_obj, include/nagp.h).  dobj is
% formed only when asked for.

  out = cell(1, max(nargout, 1));       % nlhs of the gateway = nargout: dobj is formed only when asked for
  if nargin == 2
    [out{:}] = nagp_mex('segp_obj', reshape(param(1:3), [], 1), specy(:), [], []);
  elseif nargin == 3
    [out{:}] = nagp_mex('segp_obj', reshape(param(1:2), [], 1), specy(:), varargin{1}, []);
  else
    [out{:}] = nagp_mex('segp_obj', param(1), specy(:), varargin{1}, varargin{2});
  end
  obj = out{1};
  if nargout > 1
    dobj = out{2};
  end
end
