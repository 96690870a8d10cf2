function [Fdraw,Xdraw,Sdraw,MS] = gf_ep_sample(w,x,y,ss,xt,kernel1,kernel2,num_lik_params,D,N,out,n_draws,varargin)
% GF_EP_SAMPLE - joint posterior draws of a gf_ep_modulator_nmf run ON THE GPU
%
% [Fdraw,Xdraw,Sdraw,MS] = gf_ep_sample(w,x,y,ss,xt,kernel1,kernel2,num_lik_params,D,N,out,n_draws [,seed [,sig [,z]]])
%
% w ... N as passed to gf_ep_modulator_nmf (log parameters, balance off) and `out` its sixth output (out.ttau, out.tnu).  The
% drivers of the reference draw sub_samp / mod_samp independently per time step from Eft / Varft (demo_nonstationary_filterbank.m:226-258);
% here whole state paths are drawn, correlated in time, from the Gaussian the last forward pass and the RTS smoother define: forward
% filter with the returned sites, backward sampling (nagp_ep_sample, include/nagp.h).  The draws come from the counter-based generator
% of libnagp.so keyed by seed (default 0), or from the caller's normals z (S x T x n_draws).
%   Fdraw  M x T x n_draws   H*x of every draw (rows 1..D sub-bands, D+1..D+N modulators)
%   Xdraw  S x T x n_draws   the states (computed only when asked for)
%   Sdraw  T x n_draws       sum_d a_d z_d with a = Wnmf*link(g) (sig.amp_kind 0) or its square root (1); [] without sig.
%                            sig: struct with amp_kind, link_kind (0 log(1+exp(g-shift)), 1 exp(g)), link_shift; Wnmf is filled in here
%   MS     S x T             the chain with every z = 0: the smoothed means, out.MS
% The other full-covariance drivers differ in the lines before the model only (gf_ep_modulator_nmf_constraints: nagp_unpack_constraints
% and nagp_balance; gf_ep_modulator: balance, predict_at_k1 = 1): build the model as they do and call nagp_mex('ep_sample', ...) directly.

  seed = 0; sig = []; z = [];
  if numel(varargin) >= 1 && ~isempty(varargin{1}), seed = varargin{1}; end
  if numel(varargin) >= 2, sig = varargin{2}; end
  if numel(varargin) >= 3, z = varargin{3}; end
  yall = nagp_inputs(x,y,xt);

  % log-transformed parameters (gf_ep_modulator_nmf.m:72-75); balance stays off in this variant (:80)
  n0 = num_lik_params;
  lik_param = w(1:n0);
  param1 = exp(w(n0+1:n0+3*D));
  param2 = exp(w(n0+3*D+1:n0+3*D+2*N));
  Wnmf = reshape(exp(w(n0+3*D+2*N+1:end)),[D,N]);
  [F,L,Qc,H,Pinf] = ss(x,param1,param2,kernel1,kernel2);
  model = nagp_model(F,L,Qc,H,Pinf,Wnmf,D,N,lik_param);
  if ~isempty(sig), sig.Wnmf = Wnmf; end

  if nargout > 3
    [Fdraw,Xdraw,Sdraw,MS] = nagp_mex('ep_sample', model, out.ttau, out.tnu, yall(:), 0, n_draws, seed, z, sig);
  elseif nargout > 2
    [Fdraw,Xdraw,Sdraw] = nagp_mex('ep_sample', model, out.ttau, out.tnu, yall(:), 0, n_draws, seed, z, sig);
  elseif nargout > 1
    [Fdraw,Xdraw] = nagp_mex('ep_sample', model, out.ttau, out.tnu, yall(:), 0, n_draws, seed, z, sig);
  else
    Fdraw = nagp_mex('ep_sample', model, out.ttau, out.tnu, yall(:), 0, n_draws, seed, z, sig);
  end
end
