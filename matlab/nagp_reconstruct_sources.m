function [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod] = nagp_reconstruct_sources(Eft,Varft,Wnmf,link,amplitude,sources,n_samples,seed,p_cubature)
% NAGP_RECONSTRUCT_SOURCES - the post-processing of the experiment scripts (experiments/source_sep_piano.m:165-244,
% noise_reduction_speech.m:142): sig = sum_d a_d z_d with a = sqrt(Wnmf*link(g)) ('sqrt', the model of likModulatorPreCalcwn) or
% a = Wnmf*link(g) ('linear', the demos), the per-source signals sig_j (sums over each source's sub-bands) and the envelopes
% envs = mean a, under the independent posterior marginals
%
%   [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod] = nagp_reconstruct_sources(Eft,Varft,Wnmf,link[,amplitude[,sources[,n_samples[,seed[,p_cubature]]]]])
%
% Wnmf: D x N, or a cell of per-source matrices (W_all = blkdiag(Wnmf{:}), the sources taken from it); sources: [] (one source), J
% (J equal blocks, source_sep_piano.m:221-223) or the J+1 zero-based offsets; Esrc, Vsrc: J x T (Esig1..3 / Vsig1..3), Eenv: D x T.
% n_samples = 0 (default): population values (gauher(32) per modulator; 'sqrt': the rule utp_ws(p_cubature,N) / mvhermgauss over the
% modulators, default 5); n_samples >= 2: the scripts' estimator (100 draws there) on reproducible draws.
% Only the outputs asked for are computed.
  if nargin < 5 || isempty(amplitude), amplitude = 'sqrt'; end
  if nargin < 6, sources = []; end
  if nargin < 7 || isempty(n_samples), n_samples = 0; end
  if nargin < 8 || isempty(seed), seed = 0; end
  if nargin < 9 || isempty(p_cubature), p_cubature = 5; end
  if iscell(Wnmf)
    off = 0; for j = 1:numel(Wnmf), off(end+1) = off(end) + size(Wnmf{j},1); end %#ok<AGROW>
    Wnmf = blkdiag(Wnmf{:});
  else
    D = size(Wnmf,1);
    if isempty(sources), off = [0 D];
    elseif isscalar(sources), off = (0:sources)*(D/sources);
    else, off = sources(:)';
    end
  end
  N = size(Wnmf,2);
  [link_kind,link_shift] = nagp_link(link);
  o = struct('amp_kind',double(strcmp(amplitude,'sqrt')),'link_kind',link_kind,'link_shift',link_shift,'source_offsets',int32(off), ...
             'n_samples',n_samples,'seed',seed,'device',0);
  if n_samples == 0
    [gx,gw] = gauher(32);                        % nodes / weights for the standard normal weight (reference file gauher.m)
    o.gh_x = gx(:)'; o.gh_w = gw(:)';
    if o.amp_kind == 1
      if any(p_cubature == [3 5 7 9])
        [wn,xn] = utp_ws(p_cubature,N);          % symmetric-cubature-rules/utp_ws.m
      else
        [xn,wn] = mvhermgauss(zeros(N,1),ones(N,1),p_cubature);   % Gauss-Hermite grid on the unit Gaussian
      end
      o.wn = wn(:)'; o.xn_unscaled = xn;
    end
  end
  out = cell(1,max(nargout,1));
  [out{:}] = nagp_mex('reconstruct_sources',Eft,Varft,Wnmf,o);
  out(end+1:7) = {[]};
  [Esig,Vsig,Esrc,Vsrc,Eenv,Eft_mod,Varft_mod] = deal(out{:});
end
