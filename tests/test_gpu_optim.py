"""pn2.optim.Adam / pn2.optim.SGD on the device: the one-launch kernels against the numpy float32
restatement tests/optim_ref.py bit for bit (16-byte and dword paths, every size around a chunk,
tensors off 16-byte alignment, lr changed between steps), gradients that are None or move, the
closeness to torch.optim.Adam relative to float64 at the ClsSSG parameter shapes
(profiles/optim/vs_torch.json), and a captured launch replayed with new scalars."""
import json
import os

import numpy as np
import pytest
import torch

import optim_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 2048
SIZES = (1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7)
LRS = (1e-3, 7e-4, 4.9e-4, 2e-3, 1e-5)
BETAS, EPS = (0.9, 0.999), 1e-8


def _host_data(sizes, steps, seed):
    rng = np.random.default_rng(seed)
    ps = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[(np.exp(rng.uniform(np.log(1e-4), np.log(10.0), n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
           for n in sizes] for _ in range(steps)]
    return ps, gs


def _offset_view(n, off):
    """A float32 [n] device tensor whose base is `off` elements past a 256-byte aligned
    allocation."""
    t = torch.zeros(n + 8, device=DEV)[off:off + n]
    assert t.data_ptr() % 16 == (4 * off) % 16 and t.is_contiguous()
    return t


def _make_params(ps, offsets=None):
    out = []
    for i, p in enumerate(ps):
        t = _offset_view(len(p), 0 if offsets is None else offsets[i][0])
        t.copy_(torch.from_numpy(p))
        out.append(torch.nn.Parameter(t))
    return out


def _set_grads(params, gs, offsets=None):
    for i, (p, g) in enumerate(zip(params, gs)):
        t = _offset_view(len(g), 0 if offsets is None else offsets[i][1])
        t.copy_(torch.from_numpy(g))
        p.grad = t


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _assert_bits(got, want, what):
    g, w = _bits(got), np.ascontiguousarray(want).view(np.uint32)
    assert np.array_equal(g, w), "%s: %d of %d values differ" % (what, int((g != w).sum()), g.size)


def _run_adam(sizes, steps, wd, offsets=None, seed=0):
    from pn2 import optim
    ps, gs = _host_data(sizes, steps, seed)
    params = _make_params(ps, offsets)
    opt = optim.Adam(params, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=wd)
    if offsets is not None:  # state off alignment too: created here, as load_state_dict could leave it
        for p, off in zip(params, offsets):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": _offset_view(p.numel(), off[2]),
                            "exp_avg_sq": _offset_view(p.numel(), off[3])}
    rp = [p.copy() for p in ps]
    rm = [np.zeros_like(p) for p in ps]
    rv = [np.zeros_like(p) for p in ps]
    for t in range(steps):
        opt.param_groups[0]["lr"] = LRS[t]
        _set_grads(params, gs[t], offsets)
        opt.step()
        assert opt.last_route() == "kernel"
        s = optim_ref.adam_scalars(LRS[t], BETAS, EPS, wd, t + 1)
        for i in range(len(sizes)):
            optim_ref.adam_step(rp[i], gs[t][i], rm[i], rv[i], s)
        if t in (0, steps - 1):
            for i, p in enumerate(params):
                st = opt.state[p]
                assert st["step"].item() == t + 1 and st["step"].device.type == "cpu"
                _assert_bits(p, rp[i], "p[n=%d] step %d" % (sizes[i], t + 1))
                _assert_bits(st["exp_avg"], rm[i], "exp_avg[n=%d] step %d" % (sizes[i], t + 1))
                _assert_bits(st["exp_avg_sq"], rv[i], "exp_avg_sq[n=%d] step %d" % (sizes[i], t + 1))
    return opt


@pytest.mark.parametrize("wd", (0.0, 1e-4))
def test_adam_bits_against_the_restatement(wd):
    _run_adam(SIZES, 5, wd)


# each of p, g, m, v in turn one element off 16-byte alignment (the dword path and the choice
# between the paths), on sizes with whole chunks; the first tensor stays aligned
OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (2, 0, 3, 0)]
OFF_SIZES = (2 * CHUNK, CHUNK, CHUNK + 1, 2 * CHUNK, CHUNK, 65, 2 * CHUNK + 5)


@pytest.mark.parametrize("wd", (0.0, 1e-4))
def test_adam_bits_off_alignment(wd):
    _run_adam(OFF_SIZES, 2, wd, offsets=OFFSETS, seed=3)


@pytest.mark.parametrize("offsets", (None, OFFSETS))
@pytest.mark.parametrize("mu", (0.0, 0.9))
@pytest.mark.parametrize("wd", (0.0, 1e-4))
def test_sgd_bits_against_the_restatement(wd, mu, offsets):
    from pn2 import optim
    sizes = SIZES if offsets is None else OFF_SIZES
    steps = 5
    ps, gs = _host_data(sizes, steps, 11)
    params = _make_params(ps, offsets)
    opt = optim.SGD(params, lr=0.01, momentum=mu, weight_decay=wd)
    rp = [p.copy() for p in ps]
    rb = [np.zeros_like(p) if mu else None for p in ps]
    for t in range(steps):
        lr = LRS[t] * 10
        opt.param_groups[0]["lr"] = lr
        _set_grads(params, gs[t], offsets)
        if offsets is not None and mu and t == 0:
            for p, off in zip(params, offsets):  # an existing, unaligned buffer: not the first step
                opt.state[p]["momentum_buffer"] = _offset_view(p.numel(), off[2])
        first = t == 0 and offsets is None
        opt.step()
        assert opt.last_route() == "kernel"
        s = optim_ref.sgd_scalars(lr, mu, 0.0, wd, first=first)
        for i in range(len(sizes)):
            optim_ref.sgd_step(rp[i], gs[t][i], rb[i], s)
        if t in (0, steps - 1):
            for i, p in enumerate(params):
                _assert_bits(p, rp[i], "p[n=%d] step %d" % (sizes[i], t + 1))
                if mu:
                    _assert_bits(opt.state[p]["momentum_buffer"], rb[i], "buf[n=%d] step %d" % (sizes[i], t + 1))
                else:
                    assert "momentum_buffer" not in opt.state[p]


def test_grad_none_is_untouched_and_moved_grads_refresh_the_table():
    from pn2 import optim
    sizes = (100, CHUNK + 3, 64, 5000)
    ps, gs = _host_data(sizes, 4, 21)
    params = _make_params(ps)
    opt = optim.Adam(params, lr=1e-3, weight_decay=1e-4)
    rp, rm, rv = [p.copy() for p in ps], [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    steps_of = [0] * len(sizes)
    keep = []
    for t in range(4):
        skip = {1} if t in (0, 3) else set()  # a parameter in the middle without a gradient
        if t == 2:  # the same set as step 2, but the old allocations are held: every gradient moves
            keep = [p.grad for p in params]
        _set_grads(params, gs[t])
        for i in skip:
            params[i].grad = None
        if t == 2:
            assert all(p.grad.data_ptr() != k.data_ptr() for p, k in zip(params, keep))
        before = opt.table_uploads()
        opt.step()
        assert opt.last_route() == "kernel"
        assert opt.table_uploads() == before + 1  # the set or the addresses changed every time here
        for i in range(len(sizes)):
            if i in skip:
                continue
            steps_of[i] += 1
            optim_ref.adam_step(rp[i], gs[t][i], rm[i], rv[i],
                                optim_ref.adam_scalars(1e-3, BETAS, EPS, 1e-4, steps_of[i]))
        for i, p in enumerate(params):
            _assert_bits(p, rp[i], "p[%d] step %d" % (i, t + 1))
            if steps_of[i]:
                assert opt.state[p]["step"].item() == steps_of[i]
                _assert_bits(opt.state[p]["exp_avg"], rm[i], "exp_avg[%d] step %d" % (i, t + 1))
            else:
                assert p not in opt.state
    assert steps_of == [4, 2, 4, 4]
    # gradients written in place (zero_grad(set_to_none=False)): no new upload
    before = opt.table_uploads()
    for p, g in zip(params, gs[0]):
        if p.grad is not None:
            p.grad.copy_(torch.from_numpy(g))
    opt.step()
    assert opt.table_uploads() == before
    assert opt.state[params[1]]["step"].item() == 2 and opt.state[params[0]]["step"].item() == 5


def _ulps(a, b):
    """Largest distance in float32 ulps (of b's binade) between two float32 arrays."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(b), np.float32(1e-30)).astype(np.float32)).astype(np.float64)
    return float((np.abs(a64 - b64) / ulp).max())


def test_closeness_to_torch_adam_at_the_cls_ssg_shapes():
    """Error against a float64 Adam: the kernel's at most twice torch.optim.Adam's, per state
    tensor kind over all ClsSSG parameter shapes, after 5 steps on the same device."""
    from pn2 import heads, optim
    from test_optim_ref import adam64
    shapes = [tuple(p.shape) for p in heads.ClsSSG().parameters()]
    sizes = [int(np.prod(s)) for s in shapes]
    steps, lr, wd = 5, 1e-3, 1e-4
    ps, gs = _host_data(sizes, steps, 31)
    ours = [torch.nn.Parameter(torch.from_numpy(p).to(DEV).reshape(s)) for p, s in zip(ps, shapes)]
    theirs = [torch.nn.Parameter(torch.from_numpy(p).to(DEV).reshape(s)) for p, s in zip(ps, shapes)]
    oa = optim.Adam(ours, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
    ob = torch.optim.Adam(theirs, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
    for t in range(steps):
        for p, q, g, s in zip(ours, theirs, gs[t], shapes):
            p.grad = torch.from_numpy(g).to(DEV).reshape(s)
            q.grad = p.grad.clone()
        oa.step()
        ob.step()
    assert oa.last_route() == "kernel"
    err = {k: [0.0, 0.0] for k in ("p", "exp_avg", "exp_avg_sq")}
    ulps = {k: 0.0 for k in err}
    for i, (p, q) in enumerate(zip(ours, theirs)):
        want = adam64(ps[i], [g[i] for g in gs], lr, BETAS, EPS, wd)
        got = (p, oa.state[p]["exp_avg"], oa.state[p]["exp_avg_sq"])
        ref = (q, ob.state[q]["exp_avg"], ob.state[q]["exp_avg_sq"])
        for k, a, b, w in zip(err, got, ref, want):
            a, b = a.detach().cpu().numpy().reshape(-1), b.detach().cpu().numpy().reshape(-1)
            err[k][0] = max(err[k][0], float(np.abs(a.astype(np.float64) - w).max()))
            err[k][1] = max(err[k][1], float(np.abs(b.astype(np.float64) - w).max()))
            ulps[k] = max(ulps[k], _ulps(a, b))
    record = {"shapes": "ClsSSG parameters (%d tensors, %d elements)" % (len(sizes), sum(sizes)), "steps": steps,
              "lr": lr, "weight_decay": wd,
              "max_ulps_vs_torch": ulps,
              "max_abs_error_vs_float64": {k: {"pn2": v[0], "torch": v[1]} for k, v in err.items()}}
    print(json.dumps(record))
    out = os.path.join(ROOT, "profiles", "optim")
    try:  # the record of the last run (a read-only checkout keeps the committed one)
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "vs_torch.json"), "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass
    for k, (eo, et) in err.items():
        assert eo <= 2 * et, (k, eo, et)


def test_captured_launch_replays_with_the_scalars_in_memory():
    """One launch captured, replayed 3 times with prepare_scalars() and a changed lr between the
    replays == 3 eager steps, bit for bit.  A kernel that took lr or the bias corrections by
    value would repeat the captured step's."""
    from pn2 import optim
    sizes = (5, 64, CHUNK, CHUNK + 1, 3 * CHUNK)
    ps, gs = _host_data(sizes, 5, 41)
    lrs = (1e-3, 7e-4, 3e-3, 1e-4, 5e-4)

    def build():
        params = _make_params(ps)
        opt = optim.Adam(params, lr=lrs[0], weight_decay=1e-4)
        _set_grads(params, gs[0])
        return params, opt

    def load(params, t):
        for p, g in zip(params, gs[t]):
            p.grad.copy_(torch.from_numpy(g))  # in place: the captured addresses stay

    ea, oa = build()
    for t in range(5):
        oa.param_groups[0]["lr"] = lrs[t]
        load(ea, t)
        oa.step()

    eb, ob = build()
    for t in range(2):  # two eager steps, then one captured launch replayed three times
        ob.param_groups[0]["lr"] = lrs[t]
        load(eb, t)
        ob.step()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    uploads = ob.table_uploads()
    with torch.cuda.graph(g):
        ob.step(scalars_ready=True)
    assert ob.table_uploads() == uploads  # nothing but the launch was recorded
    for t in range(2, 5):
        ob.param_groups[0]["lr"] = lrs[t]
        load(eb, t)
        assert ob.prepare_scalars()
        g.replay()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ea, eb)):
        assert oa.state[p]["step"].item() == ob.state[q]["step"].item() == 5
        _assert_bits(q, p.detach().cpu().numpy(), "p[%d]" % i)
        _assert_bits(ob.state[q]["exp_avg"], oa.state[p]["exp_avg"].cpu().numpy(), "exp_avg[%d]" % i)
        _assert_bits(ob.state[q]["exp_avg_sq"], oa.state[p]["exp_avg_sq"].cpu().numpy(), "exp_avg_sq[%d]" % i)
    # and the eager result is the restatement's
    rp, rm, rv = [p.copy() for p in ps], [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    for t in range(5):
        for i in range(len(sizes)):
            optim_ref.adam_step(rp[i], gs[t][i], rm[i], rv[i], optim_ref.adam_scalars(lrs[t], BETAS, EPS, 1e-4, t + 1))
    for i, p in enumerate(ea):
        _assert_bits(p, rp[i], "p[%d] against the restatement" % i)
