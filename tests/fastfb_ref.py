"""NumPy float64 restatement of the two loops of unifying_prob_tf/kernel_ss_kalmanFastFB.m (filter :83-110, steady-state smoother
:134-151) in the two forms nagp_fastfb_run computes them:

  sequential(setup, y, KF)   the loops as the .m writes them;
  span_form(setup, y, KF)    the parallel-in-time form of the kernels: compose every span to (Phi_j, c_j), walk the span boundaries,
                             replay every span from its boundary value; per-span sum_v2 partials added in span order.

`setup` is a mapping with the constant matrices the C ABI takes -- A, AKHA, HA, Kg and G (S x S, S x S, S, S, S x S) -- and is never
computed here, so both forms serve any affine recursion of that shape, not only a filterbank's.  spans() mirrors the span
arithmetic of nagp_fastfb_run and compose_lds_doubles() the LDS demand that decides whether spans run.  Both forms are pinned to the
60-digit fixture tests/golden/fastfb_multiprecision.npz (tools/make_fastfb_fixture.py) in tests/test_fastfb_host.py."""
import numpy as np

LDS_BYTES = 160 * 1024
SPAN_MIN_T, SPAN_STEPS, SPAN_CAP = 2048, 128, 512
VARY = 0.01


def compose_lds_doubles(S):
    """fb_compose_lds_doubles of the kernels: A, B, two (S+4) x (S+4) work matrices, three vectors"""
    return 2 * S * S + 2 * (S + 4) * (S + 4) + 3 * S + 8


def spans(T, S=1, sequential=False):
    """(ns, L, nss): filter spans, span length, smoother spans (0 when T == 1) of nagp_fastfb_run for T steps of S states"""
    ns = 1
    if compose_lds_doubles(S) * 8 <= LDS_BYTES and T >= SPAN_MIN_T and not sequential:
        ns = min(SPAN_CAP, T // SPAN_STEPS)
    L = (T + ns - 1) // ns
    ns = (T + L - 1) // L
    return ns, L, (T - 1 + L - 1) // L


def dist(a, ref):
    """the project's norm: max|a - ref| / max|ref|"""
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(a, float) - ref)) / np.max(np.abs(ref)))


def lik(Sinn, T, sum_v2):
    """kernel_ss_kalmanFastFB.m:78,97,159 -- every step counts in the constant part, observed or not"""
    return -(0.5 * np.log(2 * np.pi) * T + 0.5 * np.log(Sinn) * T + 0.5 * sum_v2 / Sinn)


def recipe(kernel, D, seed):
    """Hyper-parameters of the filterbank test models (the recipe of tests/test_gpu_parity.py): lamx, varx, omega"""
    rng = np.random.default_rng(seed)
    return 1.0 / rng.uniform(20, 400, D), rng.uniform(0.1, 1.0, D), np.linspace(np.pi / 3, np.pi / 50, D)


def simulate_y(A, Q, H, Pinf, T, seed, noise=0.1):
    """A series drawn from the model"""
    rng = np.random.default_rng(seed); S = A.shape[0]
    Lc = np.linalg.cholesky(Pinf); Lq = np.linalg.cholesky(Q + 1e-14 * np.eye(S)); H = np.ravel(H)
    z = Lc @ rng.normal(size=S); y = np.zeros(T)
    for k in range(T):
        z = A @ z + Lq @ rng.normal(size=S); y[k] = H @ z + noise * rng.normal()
    return y


def _unpack(setup):
    A = np.asarray(setup['A'], float); B = np.asarray(setup['AKHA'], float)
    G = setup.get('G')
    return A, B, np.ravel(setup['HA']).astype(float), np.ravel(setup['Kg']).astype(float), None if G is None else np.asarray(G, float)


def _filter_steps(A, B, ha, kg, y, m, ka, kb, out):
    sv2 = 0.0
    for k in range(ka, kb):
        if not np.isnan(y[k]):
            v = y[k] - ha @ m
            m = B @ m + kg * y[k]
            sv2 += v * v
        else:
            m = A @ m
        out[:, k] = m
    return sv2


def _smoother_steps(A, G, MS, m, ka, kb):
    """steps kb-1 ... ka, descending, in place"""
    for k in range(kb - 1, ka - 1, -1):
        m = MS[:, k] + G @ (m - A @ MS[:, k])
        MS[:, k] = m


def sequential(setup, y, KF=0):
    """MS (S x T; the filtered means when KF == 1) and sum_v2 = the sum of (y_k - HA m_{k-1})^2 over the observed steps"""
    A, B, ha, kg, G = _unpack(setup)
    y = np.asarray(y, float).ravel(); T = y.size; S = A.shape[0]
    MS = np.zeros((S, T))
    sv2 = _filter_steps(A, B, ha, kg, y, np.zeros(S), 0, T, MS)
    if KF != 1 and T > 1:
        _smoother_steps(A, G, MS, MS[:, T - 1].copy(), 0, T - 1)
    return MS, sv2


def span_form(setup, y, KF=0):
    """The same outputs by spans of spans(T, S): compose, boundary walk, replay."""
    A, B, ha, kg, G = _unpack(setup)
    y = np.asarray(y, float).ravel(); T = y.size; S = A.shape[0]
    ns, L, nss = spans(T, S)
    MS = np.zeros((S, T))
    # filter: m_k = M_k m_{k-1} + u_k with (M_k, u_k) = (AKHA, Kg y_k) where y_k is observed, (A, 0) where it is not
    starts = np.zeros((ns, S)); s = np.zeros(S)
    for j in range(ns):
        Phi = np.eye(S); c = np.zeros(S)
        for k in range(j * L, min((j + 1) * L, T)):
            if not np.isnan(y[k]):
                Phi = B @ Phi; c = B @ c + kg * y[k]
            else:
                Phi = A @ Phi; c = A @ c
        starts[j] = s
        s = Phi @ s + c
    sv2 = 0.0
    for j in range(ns):
        sv2 += _filter_steps(A, B, ha, kg, y, starts[j], j * L, min((j + 1) * L, T), MS)
    if KF == 1 or T < 2:
        return MS, sv2
    # smoother over the n = T-1 steps, descending: m_k = G m_{k+1} + (MS_k - G A MS_k)
    n = T - 1
    starts = np.zeros((nss, S)); s = MS[:, T - 1].copy()
    for j in range(nss - 1, -1, -1):
        Phi = np.eye(S); c = np.zeros(S)
        for k in range(min((j + 1) * L, n) - 1, j * L - 1, -1):
            Phi = G @ Phi; c = MS[:, k] + G @ (c - A @ MS[:, k])
        starts[j] = s
        s = Phi @ s + c
    for j in range(nss):
        _smoother_steps(A, G, MS, starts[j], j * L, min((j + 1) * L, n))
    return MS, sv2


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
SETUP_KEYS = ('PP', 'Sinn', 'Kg', 'HA', 'AKHA', 'PF2', 'G', 'Psm')
MODEL_OF = {'m32': 'm32', 'm52': 'm52', 'span': 'm32', 'span_wide': 'wide'}        # recursion case -> the model it runs on


def fixture_model(f, name):
    """inputs (A, Q, H, vary) and the stored set-up of model `name` of the loaded fixture `f` (keys '<name>__<array>')"""
    return {k[len(name) + 2:]: f[k] for k in f if k.startswith(name + '__')}


def fixture_case(f, name):
    """a recursion case (keys 'run_<name>__<array>'): its model's set-up plus y, steps, MF and MS at `steps`, sum_v2 and lik"""
    c = fixture_model(f, MODEL_OF[name])
    c.update({k[len(name) + 6:]: f[k] for k in f if k.startswith('run_' + name + '__')})
    return c
