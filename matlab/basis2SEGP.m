function Y = basis2SEGP(Z,lenx,varx,tol)
% BASIS2SEGP - the basis-function representation of a squared-exponential GP to the GP itself, ON THE GPU
%
% Y = basis2SEGP(Z,lenx,varx,tol)
% The argument list of experiments/toolsGP/basis2SEGP.m: Z [T,K] coefficients, lenx, varx [K,1], tol the extent of the basis functions;
% Y [T,K] = conv(Z(:,k),bas_k,'same') per column (nagp_sebf_conv, include/nagp.h).

  Y = nagp_mex('sebf_conv', Z, lenx, varx, tol);
end
