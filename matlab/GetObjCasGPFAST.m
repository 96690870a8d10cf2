function [Obj,dObjdx] = GetObjCasGPFAST(x,y,fftCovs,Params,Dims)
% GETOBJCASGPFAST - objective (and gradient) of the joint fine tuning of a GPPAD cascade, ON THE GPU
%
% [Obj,dObjdx] = GetObjCasGPFAST(x,y,fftCovs,Params,Dims)
% The argument list of experiments/gppad/Cascade/GetObjCasGPFAST.m: x [M*Tx,1] the transformed modulators X(:), y [T,1] signal, fftCovs
% [Tx,M] the prior spectra of GetFFTCovFast.m, Params with varx, mux ([M] each) and varc (len and vary are not read), Dims with T, Tx and M.
% Put ahead of the reference's file on the path, it lets the reference's FBCasGPMAP.m, CasGPMAP.m, MAPGPCasFast.m and minimize.m run
% unchanged on the device objective (nagp_gppad_cas_obj, include/nagp.h).  dObjdx is formed only when asked for.

  if numel(x) ~= Dims.M * Dims.Tx || numel(y) ~= Dims.T || size(fftCovs, 1) ~= Dims.Tx || size(fftCovs, 2) ~= Dims.M
    error('nagp:arg', 'x must hold Dims.M * Dims.Tx and y Dims.T entries, and fftCovs must be Dims.Tx x Dims.M');
  end
  out = cell(1, max(nargout, 1));       % nlhs of the gateway = nargout: dObjdx is formed only when asked for
  [out{:}] = nagp_mex('gppad_cas_obj', x(:), y(:), fftCovs, Params.varx(:), Params.mux(:), Params.varc);
  Obj = out{1};
  if nargout > 1
    dObjdx = out{2};
  end
end
