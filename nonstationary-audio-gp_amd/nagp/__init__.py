"""nagp -- host-side mirror of the reference's hot-path interface over libnagp.so (HIP, gfx950).

    from nagp import gf_ep_modulator_nmf, Mom, SSHandle
"""
from ._lib import build, lib, NagpError, LIB_PATH  # noqa: F401
from .api import (Mom, SSHandle, gf_ep_modulator, gf_ep_modulator_nmf, gf_ep_modulator_nmf_constraints,  # noqa: F401
                  ihgp_ep_modulator_nmf, ihgp_ep_modulator_nmf_constraints, gf_giekf_modulator_nmf,
                  gf_giekf_modulator_nmf_constraints, MeasModel, ekf_update1, iekf_update1,
                  gf_ep_mods_nmf_mixture, ihgp_ep_mods_nmf_mixture)
from .ss import ss_modulators, ss_modulators_nmf, lti_disc, sigmoid, inv_sigmoid  # noqa: F401
from .cubature import utp_ws, gauher, mvhermgauss_unit  # noqa: F401
from .plan import Plan, batch_run, batch_partition  # noqa: F401
from .fastfb import get_disc_model, kernel_ss_kalmanFastFB, kernel_ss_sampleFastFB  # noqa: F401
from .slowfb import kernel_ss_kalmanSlowFB, slowfb_run  # noqa: F401
from .nmf import nmf_run, nmf_fp, nmf_inf_fp, nmf_init, kernel_ss_probFB, getFBLDSOutput_tau  # noqa: F401
from .pstft import (pstft_obj, get_Obj_pSTFT_exp, get_Obj_pSTFT_matern32, get_Obj_pSTFT_matern52, get_Obj_pSTFT_all,  # noqa: F401
                    welchMethod, freq2probSpec, minimize, fit_probSTFT_SD, fit_probSTFT_SD_many)
from .segp import segp_obj, getObjSEGP, getGPSESpec, trainSEGP_RS, trainSEGP_RS_many, modulator_prior_init  # noqa: F401
from .gppad import (gppad_obj, GppadHandle, GetGPObjFast, GetFFTCovFast, GetTx, GetDSs, GetAmp, PackParamsGP, InitPADSampleNonStat,  # noqa: F401
                    LearnMarginalParams, GridMargParams, GetObjNumericalInt, GetObjNumericalInt2, ConjGradMargParams, MAPGPFast,
                    InferAmplitudeGPMAP, InferAmplitudeGPMAP_many, FBGPMAP, GPPAD, resample2)
from . import nmf_temp  # noqa: F401  (its driver `nmf` is reached as nagp.nmf_temp.nmf: nagp.nmf is the module of the fixed-point NMF)
from .nmf_temp import nmf_temp_obj, NmfTempHandle, getObj_nmf_temp, getObj_nmf_temp_inf, nmf_inf, nmf_inf_many  # noqa: F401
from .gppad_cas import (gppad_cas_obj, GppadCasHandle, GetObjCasGPFAST, PackDimsCas, UnpackDimsCas, MAPGPCasFast, CasGPMAP, FBCasGPMAP)  # noqa: F401
from .gppad_lap import (GppadLapHandle, GetHessian, SigDSigTimesV, LanczosGPPAD, GetEigSigDSig, GetErrorBarGPPAD, GetLaplaceObjGPPADOneChunk,  # noqa: F401
                        GetLaplaceObjGPPAD, GetLaplaceObjGPPADMulti, GetLaplaceObjGPPADStitched, GetLenGridSearch, GetLenGradAscent, FBGPMAPLearnLen,
                        InferAmplitudeErrorBarsGPMAP, LoadLearnLenGradAscentGPPADOpts, LoadErrorBarsLapOpts)
from . import tnmf  # noqa: F401  (its drivers are reached as nagp.tnmf.tnmf and nagp.tnmf.tnmf_inf: no top-level function shadows the module)
from .tnmf import (basis2SEGP, getObj_fitSE_basis_func, getObj_nmf_log_norm, getObj_nmf_log_norm_inf, tnmf_obj, TnmfHandle, sebf_fit_obj,  # noqa: F401
                   SebfFitHandle, fitSEGP_BF, fitSEGP_BF_many, randtnmf)
from .train import nlml_batch, fd_value_and_gradient  # noqa: F401
from .recon import reconstruct_signal, reconstruct_sources  # noqa: F401
from .epsample import gf_ep_sample, ep_sample, ep_sample_timings  # noqa: F401
