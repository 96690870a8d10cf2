"""The opt-in time-parallel schedule of the fixed-site filter (nagp_plan_set_windows, Plan(windows=...)): geometry and argument checks on the
host, and on the GPU: the option off is the plan as it was, tol = 0 re-runs every window and gives the sequential result bit for bit, and
with the default tolerance and the overlap of profiles/r07_window_contraction.txt the windowed result meets the tolerances of
tests/test_gpu_parity.py against the sequential CPU algorithm without a single re-run.

Inputs of the default-tolerance tests and what the CPU table (profiles/r07_window_contraction.txt, worst mismatch_m over its restarts; the
covariance is orders below) says about them -- the requirement is a decade under the default tolerance 1e-10, so that `reruns == 0` is a
statement about the reference alone:
  cfg2audio  T = 84 010, 4 windows, default overlap 8000:   1.7e-14 (cfg2audio rows; 3.1e-14 on the prior sample)
  cfg5seg    T = 20 000, 2 windows, default overlap 8000:   4.4e-13
  six states T = 30 000, 2 windows, overlap 12 000:         1.3e-13   (8000 steps leave 2.7e-9 there: the default overlap is NOT enough for this model)
  nlml       cfg2 model, T = 34 000, 4 windows, default overlap 8000: 3.1e-14
"""
import os
import sys

import numpy as np
import pytest

import nagp
from nagp import harness, Mom, Plan, _lib as L
from nagp import plan as nplan
from nagp import ss as pss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('Eft', 'Varft', 'MS', 'ttau', 'tnu', 'R', 'lZ', 'nlZ', 'maxDiffM', 'maxDiffP')


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-300))


# ---------------------------------------------------------------------------------------------
# host
def test_window_partition_tiles_the_fixed_site_pass_exactly():
    for T, P, Lw in ((84010, 4, 6000), (20000, 3, 6000), (1001, 7, 10), (50, 4, 0), (100000, 16, 4000)):
        ts, tw = nplan.window_partition(T, P, Lw)
        assert len(ts) == P + 1 and len(tw) == P
        assert ts[0] == 0 and ts[-1] == T - 1 and np.all(np.diff(ts) > 0)          # [0, T-1), no gap, no empty window
        assert np.max(np.diff(ts)) - np.min(np.diff(ts)) <= 1                       # equal to within a step
        assert tw[0] == 0 and np.array_equal(tw[1:], np.maximum(ts[1:-1] - Lw, 0))  # warm-up of `overlap` steps, clipped at the start


def test_window_partition_edge_cases():
    ts, tw = nplan.window_partition(5000, 1, 300)          # one window: the sequential pass
    assert list(ts) == [0, 4999] and list(tw) == [0]
    ts, tw = nplan.window_partition(5000, 0, 300)          # <= 1 means one
    assert list(ts) == [0, 4999] and list(tw) == [0]
    ts, tw = nplan.window_partition(4, 8, 2)               # T < P: one step per window, T - 1 of them
    assert list(ts) == [0, 1, 2, 3] and list(tw) == [0, 0, 0]
    ts, tw = nplan.window_partition(1, 4, 2)               # a single step: the pass is empty, one (empty) window
    assert list(ts) == [0, 0] and list(tw) == [0]
    ts, tw = nplan.window_partition(100, 4, 1000)          # T <= L: every warm-up clipped to the true start
    assert list(tw) == [0, 0, 0, 0] and ts[-1] == 99
    ts, tw = nplan.window_partition(100, 4, 30)            # clipped only where it has to be
    assert list(ts) == [0, 24, 49, 74, 99] and list(tw) == [0, 0, 19, 44]
    for bad in ((0, 4, 10), (100, 4, -1)):
        with pytest.raises(nagp.NagpError, match='invalid argument'):
            nplan.window_partition(*bad)
    lib = nagp.lib()
    assert lib.nagp_window_partition(100, 4, 10, None, None) == -1


def test_setter_argument_errors_and_refusals_are_host_checks():
    """No device is needed for any of these (this test runs on a machine without one): the C entry points refuse a null plan, and the
    Python layer makes the setter's checks -- family, overlap, tolerance -- before it creates the plan."""
    lib = nagp.lib()
    assert lib.nagp_plan_set_windows(None, 4, 100, 1e-8) == -1
    assert lib.nagp_plan_window_stats(None, None) == -1
    pr = harness.nmf_problem(3, 2, 40, 1)
    blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52')
    probs = [(blk, pr['W'], np.log(pr['w_lik']))]
    mom = Mom('likModulatorNMFPower', p_cubature=5)
    for kind in (L.KIND_IHGP, L.KIND_GIEKF):
        with pytest.raises(nagp.NagpError, match=r'unsupported shape \(-2\).*windows'):
            Plan(kind, probs, 40, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2, windows=4)
    with pytest.raises(nagp.NagpError, match=r'invalid argument \(-1\)'):
        Plan(L.KIND_GF_EP, probs, 40, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2, windows=4, window_overlap=-1)
    with pytest.raises(nagp.NagpError, match=r'invalid argument \(-1\)'):
        Plan(L.KIND_GF_EP, probs, 40, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2, windows=4, window_tol=-1e-9)
    with pytest.raises(nagp.NagpError, match=r'invalid argument \(-1\)'):
        Plan(L.KIND_GF_EP, probs, 40, mom=mom, ep_fraction=0.5, ep_damping=0.5 * np.ones(2), ep_itts=2, windows=4, window_tol=float('nan'))
    with pytest.raises(nagp.NagpError, match='windows'):
        Plan(L.KIND_GIEKF, probs, 40, ep_itts=1, l_iter=1, mode=L.MODE_NLML, windows=2)
    assert nplan.WINDOW_OVERLAP >= 0 and nplan.WINDOW_TOL > 0


# ---------------------------------------------------------------------------------------------
# GPU
def _problem(D, N, T, seed, k1='matern32', recipe='demo_nmf', balance=False):
    pr = harness.nmf_problem(D, N, T, seed, recipe, kernel1=k1)
    blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], k1, 'matern52')
    if balance:
        blk = pss.balance_blocks(blk)
    return pr, (blk, pr['W'], np.log(pr['w_lik']))


def _run(probs, ys, T, p=7, itts=2, damping=0.5, mode=L.MODE_PREDICT, want_MS=True, **win):
    plan = Plan(L.KIND_GF_EP, probs, T, mom=Mom('likModulatorNMFPower', p_cubature=p), ep_fraction=0.5, ep_damping=damping * np.ones(itts),
                ep_itts=itts, mode=mode, **win)
    try:
        plan.upload(ys); plan.execute()
        return plan.download(want_MS=want_MS), plan.window_stats(), plan.timings()
    finally:
        plan.close()


def _bit_diff(a, b, fields=FIELDS):
    return [f for f in fields if getattr(a, f) is not None and not np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True)]


@pytest.mark.gpu
def test_option_unset_or_one_window_is_the_plan_as_it_was(nagp_lib):
    T = 3000
    pr, prob = _problem(6, 2, T, 42)
    y = pr['y'].copy(); y[700:705] = np.nan
    (base,), st0, _ = _run([prob], [y], T, itts=3)
    assert st0 == dict(windows_run=0, boundaries_checked=0, reruns=0, warmup_steps=0, worst_m=0.0, worst_P=0.0)
    for win in (dict(windows=1), dict(windows=0), dict(windows=1, window_overlap=500, window_tol=0.0)):
        (o,), st, _ = _run([prob], [y], T, itts=3, **win)
        assert _bit_diff(o, base) == [] and np.array_equal(o.counters, base.counters), win
        assert st == st0
    # set, then taken back before the execute: the same again; and the statistics belong to the LAST execute
    plan = Plan(L.KIND_GF_EP, [prob], T, mom=Mom('likModulatorNMFPower', p_cubature=7), ep_fraction=0.5, ep_damping=0.5 * np.ones(3), ep_itts=3,
                windows=4, window_overlap=300)
    plan.upload([y]); plan.execute()
    assert plan.window_stats()['windows_run'] == 8
    plan.set_windows(1); plan.execute()
    o = plan.download()[0]
    assert plan.window_stats() == st0 and _bit_diff(o, base) == []
    # the C setter itself refuses the other families (the Python layer checks before it creates a plan: go around it)
    plan.close()
    for kind, kw in ((L.KIND_GIEKF, dict(l_iter=1)), (L.KIND_IHGP, dict(mom=Mom('likModulatorNMFPower', p_cubature=7), ep_damping=0.5 * np.ones(3)))):
        blk = pss.balance_blocks(prob[0]) if kind == L.KIND_IHGP else prob[0]
        pl = Plan(kind, [(blk, prob[1], prob[2])], T, ep_fraction=0.5, ep_itts=3, **kw)
        try:
            assert nagp_lib.nagp_plan_set_windows(pl._h, 4, 100, 1e-8) == -2
            assert nagp_lib.nagp_plan_set_windows(pl._h, 1, 100, 1e-8) == 0          # (nothing to turn off)
        finally:
            pl.close()
    pl = Plan(L.KIND_GF_EP, [prob], T, mom=Mom('likModulatorNMFPower', p_cubature=7), ep_fraction=0.5, ep_damping=0.5 * np.ones(3), ep_itts=3)
    try:
        assert nagp_lib.nagp_plan_set_windows(pl._h, 4, -1, 1e-8) == -1 and nagp_lib.nagp_plan_set_windows(pl._h, 4, 10, -1.0) == -1
    finally:
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize('k1,D,N,mode', [('matern32', 6, 2, L.MODE_PREDICT), ('matern52', 4, 2, L.MODE_PREDICT), ('matern32', 16, 3, L.MODE_PREDICT),
                                         ('matern32', 32, 6, L.MODE_PREDICT),      # S = 146: the wide one-tile-per-thread kernel, column-owner smoother
                                         ('matern32', 6, 2, L.MODE_NLML)])
def test_tol_zero_reruns_every_window_and_equals_the_sequential_schedule_bit_for_bit(k1, D, N, mode, nagp_lib):
    """tol = 0: every boundary fails, every window runs again from the stored state -- the re-run path -- and since nothing a warm-up or a
    discarded window did may survive, every output equals the sequential schedule's.  4 windows, 2 sweeps (one windowed pass; nlml mode: 3,
    where the last sweep has no filter): reruns == 3.  A NaN gap lies across the second boundary, one in a warm-up."""
    T, P, Lw = 3001, 4, 200
    itts = 3 if mode == L.MODE_NLML else 2
    pr, prob = _problem(D, N, T, 77, k1)
    pr2, prob2 = _problem(D, N, T, 78, k1)
    ts, _ = nplan.window_partition(T, P, Lw)
    ys = [pr['y'].copy(), pr2['y'].copy()]
    ys[0][ts[2] - 6:ts[2] + 5] = np.nan; ys[0][ts[3] - 150:ts[3] - 140] = np.nan; ys[1][ts[1] - 1:ts[1] + 1] = np.nan
    seq, st0, _ = _run([prob, prob2], ys, T, itts=itts, mode=mode)
    win, st, _ = _run([prob, prob2], ys, T, itts=itts, mode=mode, windows=P, window_overlap=Lw, window_tol=0.0)
    assert st['reruns'] == P - 1 and st['windows_run'] == P and st['boundaries_checked'] == P - 1 and st['warmup_steps'] == (P - 1) * Lw
    assert st['worst_m'] > 0 and st['worst_P'] > 0          # (200 steps from the prior are nowhere near the true state)
    for q in range(2):
        assert _bit_diff(win[q], seq[q]) == [], q
        assert np.array_equal(win[q].counters, seq[q].counters), q          # (NaN observations counted once: a warm-up counts nothing)
    if mode == L.MODE_PREDICT:      # three sweeps: two windowed passes
        seq3, _, _ = _run([prob], ys[:1], T, itts=3)
        win3, st3, _ = _run([prob], ys[:1], T, itts=3, windows=P, window_overlap=Lw, window_tol=0.0)
        assert st3['reruns'] == 2 * (P - 1) and _bit_diff(win3[0], seq3[0]) == []


def _tolerances():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_parity import TOL_MEAN, TOL_SITE, TOL_LOGZ
    return TOL_MEAN, TOL_SITE, TOL_LOGZ


def _report(name, st, tim_seq, tim_win, diffs):
    print('\n[windows] %s: %s\n[windows] %s: filter_lin %.1f -> %.1f ms, execute %.1f -> %.1f ms; windowed vs sequential: %s' % (
        name, st, name, tim_seq['ms']['filter_lin'], tim_win['ms']['filter_lin'], tim_seq['total_ms'], tim_win['total_ms'],
        ', '.join('%s %.2e' % kv for kv in diffs.items())))


@pytest.mark.gpu
@pytest.mark.parametrize('name,P', [('cfg2audio', 4), ('cfg5seg', 2)])
def test_full_length_shapes_with_default_tolerance_meet_the_parity_tolerances_without_a_rerun(name, P, full_length_refs):
    """The inputs of the full-length parity tests, all three sweeps, windows with the default overlap and tolerance, against the sequential
    CPU algorithm at the tolerances of tests/test_gpu_parity.py.  The table (module docstring) puts the boundary mismatch a decade and more
    under the tolerance, so no window may run again."""
    TOL_MEAN, TOL_SITE, TOL_LOGZ = _tolerances()
    flp = full_length_refs.mod
    assert (flp.TOL_MEAN, flp.TOL_SITE, flp.TOL_LOGZ) == (TOL_MEAN, TOL_SITE, TOL_LOGZ)
    full_length_refs.start()
    c = flp.CASES[name]; pr = full_length_refs.problems[name]; T = pr['y'].size
    blk = pss.ss_blocks_nmf(pr['param1'], pr['param2'], 'matern32', 'matern52')
    if c['balance']:
        blk = pss.balance_blocks(blk)
    prob = (blk, pr['W'], np.log(pr['w_lik']))
    ts, tw = nplan.window_partition(T, P, nplan.WINDOW_OVERLAP)
    assert np.all(ts[1:-1] - tw[1:] == nplan.WINDOW_OVERLAP) and nplan.WINDOW_OVERLAP < T // P      # full warm-ups, shorter than a window
    kw = dict(p=c['p'], itts=flp.SWEEPS, damping=c.get('damping', 0.5), want_MS=False)
    (seq,), _, tim_seq = _run([prob], [pr['y']], T, **kw)
    (win,), st, tim_win = _run([prob], [pr['y']], T, windows=P, **kw)
    _report('%s T=%d P=%d L=%d' % (name, T, P, nplan.WINDOW_OVERLAP), st, tim_seq, tim_win,
            {f: rel(getattr(win, f), getattr(seq, f)) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'nlZ')})
    assert st['windows_run'] == 2 * P and st['boundaries_checked'] == 2 * (P - 1)
    ref = full_length_refs.result(name)
    assert ref['status'] == 0
    m = flp.compare(name, win, ref)
    bad = {k: v for k, (v, tol) in m.items() if tol is not None and not v <= tol}
    assert not bad, (name, bad)
    assert st['reruns'] == 0, st
    assert st['worst_m'] <= nplan.WINDOW_TOL and st['worst_P'] <= nplan.WINDOW_TOL


@pytest.mark.gpu
def test_six_state_blocks_windowed_against_the_oracle_without_a_rerun():
    """Split blocks (Matern-5/2 sub-bands: six states over two tile rows, the CPL instantiations): D = 8, N = 3, T = 30 000, two windows.
    This model forgets more slowly (table: 2.7e-9 after 8000 steps, 1.3e-13 after 12 000): overlap 12 000, default tolerance."""
    from oracle import gf_ep as ogf, lik as olik
    TOL_MEAN, TOL_SITE, TOL_LOGZ = _tolerances()
    D, N, T, P, Lw = 8, 3, 30000, 2, 12000
    pr, prob = _problem(D, N, T, 11, 'matern52')
    y = pr['y'].copy(); y[14990:15012] = np.nan          # a gap of missing observations across the boundary (t_1 = 14 999)
    assert list(nplan.window_partition(T, P, Lw)[0]) == [0, 14999, 29999]
    kw = dict(p=7, itts=2, damping=0.1)
    (seq,), _, tim_seq = _run([prob], [y], T, **kw)
    (win,), st, tim_win = _run([prob], [y], T, windows=P, window_overlap=Lw, **kw)
    _report('sixstate T=%d P=%d L=%d' % (T, P, Lw), st, tim_seq, tim_win, {f: rel(getattr(win, f), getattr(seq, f)) for f in ('Eft', 'Varft', 'ttau', 'tnu', 'nlZ')})
    t = np.arange(1, T + 1.0)
    o = ogf.gf_ep_modulator_nmf(pr['w'], t, y, None, olik.Mom(olik.LIK_POWER_NMF, p=7), t, 'matern52', 'matern52', 1, D, N, 0.5, 0.1 * np.ones(2), 2)
    assert rel(win.Eft, o[0]) < TOL_MEAN and rel(win.Varft, o[1]) < TOL_MEAN
    assert rel(win.ttau, o[5]['ttau']) < TOL_SITE and rel(win.tnu, o[5]['tnu']) < TOL_SITE
    assert np.max(np.abs(win.nlZ - o[5]['nlZ']) / np.abs(o[5]['nlZ'])) < TOL_LOGZ
    assert st['windows_run'] == P and st['reruns'] == 0, st


def _oracle_nlml(args):
    w, y, D, N, p, damping, itts = args
    sys.path.insert(0, ROOT)
    from oracle import gf_ep as ogf, lik as olik
    model = ogf.build_model_nmf(w, 'matern32', 'matern52', 1, D, N, False)
    return ogf.run_nlml(model, y, olik.Mom(olik.LIK_POWER_NMF, p=p), 0.5, damping * np.ones(itts), itts)[0]


@pytest.mark.gpu
def test_nlml_mode_and_the_batched_objective_with_windows():
    """Likelihood mode (three sweeps: the fixed-site filter is the one of sweep 2) on the cfg2 model, T = 34 000, four windows with the
    default overlap and tolerance: the plan, and nlml_batch(..., windows=4) with three replicas, against the NumPy oracle's run_nlml
    (three processes beside the GPU work) at the log-Z tolerance of tests/test_gpu_parity.py; no window runs again."""
    import multiprocessing as mp
    _, _, TOL_LOGZ = _tolerances()
    D, N, T, P, itts, d = 16, 3, 34000, 4, 3, 0.5
    pr, prob = _problem(D, N, T, 1000)
    rng = np.random.default_rng(5)
    ws = [pr['w'], pr['w'] + 0.01 * rng.standard_normal(pr['w'].size), pr['w'] + 0.01 * rng.standard_normal(pr['w'].size)]
    assert nplan.WINDOW_OVERLAP < T // P
    with mp.get_context('spawn').Pool(3) as pool:
        fut = pool.map_async(_oracle_nlml, [(w, pr['y'], D, N, 9, d, itts) for w in ws])
        (seq,), _, _ = _run([prob], [pr['y']], T, p=9, itts=itts, damping=d, mode=L.MODE_NLML)
        (win,), st, _ = _run([prob], [pr['y']], T, p=9, itts=itts, damping=d, mode=L.MODE_NLML, windows=P)
        t = np.arange(1, T + 1.0)
        mom = Mom('likModulatorNMFPower', p_cubature=9)
        f_seq = nagp.nlml_batch(ws, t, pr['y'], nagp.SSHandle(), mom, 'matern32', 'matern52', 1, D, N, 0.5, d * np.ones(itts), itts)
        f_win = nagp.nlml_batch(ws, t, pr['y'], nagp.SSHandle(), mom, 'matern32', 'matern52', 1, D, N, 0.5, d * np.ones(itts), itts, windows=P)
        print('\n[windows] nlml cfg2 model T=%d P=%d L=%d: %s; windowed vs sequential edata: plan %.2e, batch %s' % (
            T, P, nplan.WINDOW_OVERLAP, st, abs(win.nlZ[0] - seq.nlZ[0]) / abs(seq.nlZ[0]), np.abs(f_win - f_seq) / np.abs(f_seq)))
        ref = np.array(fut.get(timeout=1500))
    assert st['windows_run'] == P and st['boundaries_checked'] == P - 1 and st['reruns'] == 0, st
    assert abs(win.nlZ[0] - ref[0]) / abs(ref[0]) < TOL_LOGZ
    assert np.all(np.abs(f_win - ref) / np.abs(ref) < TOL_LOGZ), (f_win, ref)


@pytest.mark.gpu
def test_function_interfaces_pass_windows_through():
    """gf_ep_modulator_nmf / _constraints / gf_ep_modulator / gf_ep_mods_nmf_mixture with windows=: short sequences, where every warm-up is
    clipped to the true start (T <= overlap) -- each window then repeats the filter from step 0 and its boundary state is the stored one
    exactly, so the outputs equal the unwindowed call bit for bit whatever the tolerance."""
    from nagp import SSHandle
    T = 600
    t = np.arange(1, T + 1.0)
    pr = harness.nmf_problem(5, 2, T, 9)
    mom = Mom('likModulatorNMFPower', p_cubature=5); d = 0.5 * np.ones(2)
    a = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, 5, 2, 0.5, d, 2, nargout=6)
    b = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, 5, 2, 0.5, d, 2, nargout=6, windows=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[5]['ttau'], b[5]['ttau']) and np.array_equal(a[5]['nlZ'], b[5]['nlZ'])
    e0, _ = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, None, 'matern32', 'matern52', 1, 5, 2, 0.5, 0.5 * np.ones(3), 3)
    e1, _ = nagp.gf_ep_modulator_nmf(pr['w'], t, pr['y'], SSHandle(), mom, None, 'matern32', 'matern52', 1, 5, 2, 0.5, 0.5 * np.ones(3), 3, windows=3)
    assert e0 == e1
    cons = harness.CONSTRAINTS_DEMO(5); tune = harness.TUNE_DEMO
    prc = harness.nmf_problem(5, 2, T, 9, 'constraints')
    w, wf = harness.constrained_vectors(prc, cons, tune)
    a = nagp.gf_ep_modulator_nmf_constraints(w, t, prc['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, 5, 2, 0.5, d, 2, cons, wf, tune)
    b = nagp.gf_ep_modulator_nmf_constraints(w, t, prc['y'], SSHandle(), mom, t, 'matern32', 'matern52', 1, 5, 2, 0.5, d, 2, cons, wf, tune, windows=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c1 = harness.cfg1(T=T)
    pm = Mom('likModulatorPower', p_cubature=9); ssh = SSHandle('ss_modulators')
    a = nagp.gf_ep_modulator(c1['w'], t, c1['y'], ssh, pm, t, 'matern32', 'matern52', 1, 0.5, 0.3 * np.ones(2), 2)
    b = nagp.gf_ep_modulator(c1['w'], t, c1['y'], ssh, pm, t, 'matern32', 'matern52', 1, 0.5, 0.3 * np.ones(2), 2, windows=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    mx = harness.mixture_problem([(3, 2), (2, 1)], T, 5, ['matern32', 'matern32'], ['matern52', 'matern52'])
    a = nagp.gf_ep_mods_nmf_mixture(mx['w'], t, mx['y'], SSHandle(), mom, t, mx['kernel1'], mx['kernel2'], mx['J'], 0.5, 0.1, 3)
    b = nagp.gf_ep_mods_nmf_mixture(mx['w'], t, mx['y'], SSHandle(), mom, t, mx['kernel1'], mx['kernel2'], mx['J'], 0.5, 0.1, 3, windows=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
