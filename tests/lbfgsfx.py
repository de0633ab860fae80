"""Fixtures of the LBFGS-polish tests (test_lbfgs_polish_host.py, test_gpu_lbfgs_polish.py): the host entry points of the
library on hparamfx records, the proxy in torch float64 with autograd, and torch.optim.LBFGS driven as the reference's
torch_minimize drives it (lib/metrics/utils.py:129-141)."""
import ctypes

import numpy as np

from tests import hparamfx as fx

OUTER_STEPS = 20
THREADS = 256          # lbp::THREADS (csrc/lbfgs_core.hpp): thread t owns the rows t, t + THREADS, ...


def polishes(ks, force_zero=(), force_one=(), starts=fx.STARTS):
    """(x0 [S,6] float64, spec [S,3] int32) in ops.lbfgs_polish's order: for each k, for each x0."""
    x0 = [[float(v) for v in s] for _ in ks for s in starts]
    spec = [[k, fx.mask(force_zero), fx.mask(force_one)] for k in ks for _ in starts]
    return np.asarray(x0, np.float64).reshape(-1, 6), np.asarray(spec, np.int32).reshape(-1, 3)


def result_tuple(r):
    return (np.array(list(r.x), np.float64), float(r.loss), int(r.nfev), int(r.nit), int(r.status))


class HostPolish(fx.HostRecord):
    """lemon_lbfgs_proxy_host and lemon_lbfgs_polish_host on a record."""

    def proxy(self, k, force_zero=(), force_one=()):
        fz, fo = fx.mask(force_zero), fx.mask(force_one)

        def f(x):
            x = np.ascontiguousarray(x, np.float64)
            grad = np.full(6, np.nan)
            loss = self.lib.lemon_lbfgs_proxy_host(*[fx._p(a) for a in self.arrs], fx._p(self.y), self.n, self.kmax, int(k), fz, fo,
                                                   fx._p(x), fx._p(grad))
            return loss, grad
        return f

    def polish_rc(self, x0, spec, outer_steps=OUTER_STEPS):
        from lemon_amd import _lib
        x0 = np.ascontiguousarray(x0, np.float64)
        spec = np.ascontiguousarray(spec, np.int32)
        S = spec.shape[0]
        out = (_lib.PolishResult * max(S, 1))()
        rc = self.lib.lemon_lbfgs_polish_host(*[fx._p(a) for a in self.arrs], fx._p(self.y), self.n, self.kmax, S, fx._p(x0),
                                              fx._p(spec), int(outer_steps), ctypes.byref(out))
        return rc, out, S

    def polish(self, x0, spec, outer_steps=OUTER_STEPS):
        from lemon_amd import _lib
        rc, out, S = self.polish_rc(x0, spec, outer_steps)
        _lib.check(rc, "lemon_lbfgs_polish_host")
        return [result_tuple(out[s]) for s in range(S)]


    def polish_parallel(self, x0, spec, outer_steps=OUTER_STEPS, workers=8):
        """polish(), one call per polish from a few Python threads (ctypes releases the GIL; the polishes are independent)"""
        from concurrent.futures import ThreadPoolExecutor
        x0, spec = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(spec, np.int32)
        with ThreadPoolExecutor(max_workers=workers) as pool:
            return list(pool.map(lambda s: self.polish(x0[s:s + 1], spec[s:s + 1], outer_steps)[0], range(spec.shape[0])))


def torch_proxy(rec, y, k, x, force_zero=(), force_one=()):
    """(loss, grad [6]) of the proxy by autograd, float64 throughout: SoftMarginLoss of the score with one exp per element."""
    import torch
    from lemon_amd.metrics import unpack_vector
    x = torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=True)
    t = {key: torch.as_tensor(np.asarray(rec[key], np.float32)).double() for key in fx.REC_KEYS}
    hp = unpack_vector(x, force_zero, force_one)
    side = lambda s: (torch.exp(-(hp["tau_1_" + s] * t["D_" + s][:, :k] + hp["tau_2_" + s] * t["dists_tr_" + s][:, :k]))
                      * t["dists_" + s][:, :k]).sum(1) / k
    score = t["d_1"] + hp["beta"] * side("n") + hp["gamma"] * side("m")
    target = torch.as_tensor(np.asarray(y).astype(bool).astype(np.float64)) * 2 - 1
    loss = torch.nn.SoftMarginLoss()(score, target)
    loss.backward()
    return float(loss.detach()), x.grad.numpy().copy()


def torch_lbfgs(value_and_grad, x0, outer_steps=OUTER_STEPS, trace=None):
    """torch.optim.LBFGS as torch_minimize sets it up (lr 0.1, max_iter 20, strong_wolfe; float64, CPU) on a function given as
    value_and_grad(x numpy [6]) -> (loss, grad).  -> (x, nfev); trace (a list) receives x after every outer step."""
    import torch
    x = torch.tensor(np.asarray(x0, np.float64), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([x], lr=0.1, max_iter=20, line_search_fn="strong_wolfe")

    def closure():
        loss, grad = value_and_grad(x.detach().numpy().copy())
        x.grad = torch.as_tensor(np.asarray(grad, np.float64)).clone()
        return torch.tensor(float(loss), dtype=torch.float64)

    for _ in range(outer_steps):
        opt.step(closure)
        if trace is not None:
            trace.append(x.detach().numpy().copy())
    return x.detach().numpy().copy(), int(opt.state[x]["func_evals"])


def rel_gap(got, want):
    """largest |got - want| / max(1, |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
