"""What the drivers of the fits share: options, the pump of a generator against an evaluator, the lock-step drivers of many generators
on one batched evaluator, and the base of the resident handles.  A driver is a generator that yields a request and is sent the answer;
its return value is the result of the fit.  A problem's bits do not depend on its batch mates, so the lock-step results equal the
one-at-a-time runs to the bit."""
import numpy as np

from . import _lib as L


def opt(opts, name, default):
    return default if not opts or name not in opts else opts[name]


def run(gen, answer):
    """pump a generator to its return value: every request it yields is sent answer(request)"""
    try:
        req = next(gen)
        while True:
            req = gen.send(answer(req))
    except StopIteration as e:
        return e.value


def forward(inner, wrap):
    """for `yield from` inside a driver: the requests of the inner generator go out as wrap(request), the answers go in as they come"""
    try:
        req = next(inner)
        while True:
            req = inner.send((yield wrap(req)))
    except StopIteration as e:
        return e.value


def lock_step(gens, key, issue):
    """the generators in lock-step: the pending requests of a round are grouped by key(request), every group is one
    issue(requests) -> one answer per request, and the answers go back.  Returns the generators' return values."""
    out = [None] * len(gens); pending = {}

    def step(into, k, a):
        try:
            into[k] = gens[k].send(a)
        except StopIteration as e:
            out[k] = e.value
    for k in range(len(gens)):
        step(pending, k, None)
    while pending:
        groups = {}
        for k, r in pending.items():
            groups.setdefault(key(r), []).append(k)
        answers = {}
        for ks in groups.values():
            answers.update(zip(ks, issue([pending[k] for k in ks])))
        pending = {}
        for k, a in answers.items():
            step(pending, k, a)
    return out


def lock_step_rows(f, gens, nx, point=lambda r: r):
    """the generators in lock-step on ONE resident evaluator f(X) -> (Obj, dObj), generator j on row j of X (n, nx): a round is one
    f(X); a generator that has left rides along with its last point.  Every generator is first resumed with None.  point(request): the
    row the request asks for, or None when the request is not a point of this evaluator -- the generator then leaves with that request
    pending.  Returns (out, left): the return values of the generators that finished, and {j: request} of those that left."""
    X = np.zeros((len(gens), nx)); out = [None] * len(gens); left = {}; live = set()

    def step(j, a):
        live.discard(j)
        try:
            r = gens[j].send(a)
        except StopIteration as e:
            out[j] = e.value
            return
        x = point(r)
        if x is None:
            left[j] = r
        else:
            X[j] = x; live.add(j)
    for j in range(len(gens)):
        step(j, None)
    while live:
        Obj, dObj = f(X)
        for j in sorted(live):
            step(j, (Obj[j], dObj[j]))
    return out, left


class ResidentHandle:
    """base of the resident forms (nagp_*_create / _eval / _destroy): a subclass sets _h, P, nx and names its C functions"""
    _h = None; _eval = _destroy = None

    def eval(self, x, grad=True):
        x = L.f64(np.asarray(x, float).reshape(self.P, self.nx), 'C')
        Obj = np.zeros(self.P); dObj = np.zeros((self.P, self.nx)) if grad else None
        if not self._h:
            raise L.NagpError('the handle is closed')
        L.check(getattr(L.lib(), self._eval)(self._h, L.dptr(x), L.dptr(Obj), L.dptr(dObj)))
        return (Obj, dObj) if grad else Obj

    def close(self):
        if self._h:
            getattr(L.lib(), self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def close(f):
    if f is not None and hasattr(f, 'close'):
        f.close()
