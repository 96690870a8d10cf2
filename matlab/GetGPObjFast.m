function [Obj,dObjdx] = GetGPObjFast(x,y,fftCov,Params,Dims)
% GETGPOBJFAST - objective (and gradient) of the GPPAD envelope inference, ON THE GPU
%
% [Obj,dObjdx] = GetGPObjFast(x,y,fftCov,Params,Dims)
% The argument list of experiments/gppad/GPModelFast/GetGPObjFast.m: x [Tx,1] transformed envelopes, y [T,1] signal, fftCov [Tx,1] the
% prior spectrum of GetFFTCovFast.m, Params with varx, mux, varc and vary (a scalar or [T,1]; len is not read), Dims with T and Tx.
% Put ahead of the reference's file on the path, it lets the reference's GPPAD.m, FBGPMAP.m, InferAmplitudeGPMAP.m, MAPGPFast.m and
% minimize.m run unchanged on the device objective (nagp_gppad_obj, include/nagp.h).  dObjdx is formed only when asked for.

  if numel(x) ~= Dims.Tx || numel(y) ~= Dims.T
    error('nagp:arg', 'x must hold Dims.Tx and y Dims.T entries');
  end
  out = cell(1, max(nargout, 1));       % nlhs of the gateway = nargout: dObjdx is formed only when asked for
  [out{:}] = nagp_mex('gppad_obj', x(:), y(:), fftCov(:), Params.varx, Params.mux, Params.varc, Params.vary(:));
  Obj = out{1};
  if nargout > 1
    dObjdx = out{2};
  end
end
