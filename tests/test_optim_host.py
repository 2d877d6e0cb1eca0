"""pn2.optim.Adam / pn2.optim.SGD on CPU tensors -- the route through super().step(): torch's
state layout, state dicts both ways, a torch checkpoint continued bit for bit, StepLR, closures,
and the route selection."""
import copy

import pytest
import torch

from pn2 import optim

KINDS = {
    "adam": (optim.Adam, torch.optim.Adam, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)),
    "sgd": (optim.SGD, torch.optim.SGD, dict(lr=0.01, momentum=0.9)),
}
SHAPES = ((5, 3), (7,), (2, 3, 4))


def _params(seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in SHAPES]


def _grads(params, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        d = torch.randn(p.shape, generator=g, dtype=p.dtype)
        p.grad = None if i in skip else d


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _state_equal(sa, sb):
    assert sa["param_groups"] == sb["param_groups"]
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        for name, t in sa["state"][k].items():
            u = sb["state"][k][name]
            assert t.dtype == u.dtype and t.device == u.device and torch.equal(t, u), (k, name)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_cpu_steps_are_torchs_and_state_layout_is_torchs(kind):
    ours_cls, torch_cls, kw = KINDS[kind]
    a, b = _params(), _params()
    oa, ob = ours_cls(a, **kw), torch_cls(b, **kw)
    assert isinstance(oa, torch_cls) and oa.last_route() is None
    for s in range(3):
        _grads(a, 10 + s)
        _grads(b, 10 + s)
        oa.step()
        ob.step()
        assert oa.last_route() == "torch"
    assert _same(a, b)
    _state_equal(oa.state_dict(), ob.state_dict())
    if kind == "adam":
        st = oa.state[a[0]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].item() == 3.0
    else:
        assert set(oa.state[a[0]]) == {"momentum_buffer"}


@pytest.mark.parametrize("direction", ("torch_to_pn2", "pn2_to_torch"))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_state_dict_round_trip_continues_bit_for_bit(kind, direction):
    ours_cls, torch_cls, kw = KINDS[kind]
    first, second = (torch_cls, ours_cls) if direction == "torch_to_pn2" else (ours_cls, torch_cls)
    a, b = _params(), _params()
    oa = first(a, **kw)       # keeps going on its own
    ob = first(b, **kw)       # is checkpointed and continued by the other class
    for s in range(2):
        for ps, o in ((a, oa), (b, ob)):
            _grads(ps, 20 + s)
            o.step()
    # what the reference's save_data writes: optimizer.state_dict() (through torch.save there)
    ckpt = copy.deepcopy(ob.state_dict())
    c = [torch.nn.Parameter(p.detach().clone()) for p in b]
    oc = second(c, **kw)
    oc.load_state_dict(ckpt)
    _state_equal(oc.state_dict(), ob.state_dict())
    for s in range(2):
        for ps, o in ((a, oa), (c, oc)):
            _grads(ps, 30 + s)
            o.step()
    assert _same(a, c)
    _state_equal(oc.state_dict(), oa.state_dict())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_steplr_drives_lr(kind):
    ours_cls, torch_cls, kw = KINDS[kind]
    a, b = _params(), _params()
    oa, ob = ours_cls(a, **kw), torch_cls(b, **kw)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.7)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.7)
    for s in range(5):
        _grads(a, 40 + s)
        _grads(b, 40 + s)
        oa.step()
        ob.step()
        sa.step()
        sb.step()
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
    assert oa.param_groups[0]["lr"] == pytest.approx(kw["lr"] * 0.7 ** 2)
    assert _same(a, b)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_grad_none_is_skipped_and_closure_is_honoured(kind):
    ours_cls, torch_cls, kw = KINDS[kind]
    a, b = _params(), _params()
    oa, ob = ours_cls(a, **kw), torch_cls(b, **kw)
    calls = []

    def closure_for(ps):
        def closure():
            assert torch.is_grad_enabled()
            calls.append(1)
            _grads(ps, 50, skip=(1,))
            return torch.tensor(3.5)
        return closure

    la, lb = oa.step(closure_for(a)), ob.step(closure_for(b))
    assert la.item() == lb.item() == 3.5 and len(calls) == 2
    assert _same(a, b)
    assert a[1] not in oa.state  # no gradient: no state, no step
    _state_equal(oa.state_dict(), ob.state_dict())


def test_route_selection_reports_torch_for_what_the_kernel_does_not_implement():
    # (on CPU every step is the torch route; the option and dtype checks are what _collect and
    # _options_ok decide before looking at the device)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict()):
        ps = _params()
        o = optim.Adam(ps, lr=1e-3, **kw)
        assert o._options_ok(o.param_groups[0]) == (not kw)
        _grads(ps, 1)
        o.step()
        assert o.last_route() == "torch"
    for kw, ok in ((dict(momentum=0.9, nesterov=True), False), (dict(maximize=True), False),
                   (dict(momentum=0.9), True), (dict(), True)):
        ps = _params()
        o = optim.SGD(ps, lr=0.1, **kw)
        assert o._options_ok(o.param_groups[0]) == ok
        _grads(ps, 1)
        o.step()
        assert o.last_route() == "torch"
    ps = _params(dtype=torch.float64)
    o = optim.Adam(ps, lr=1e-3)
    _grads(ps, 1)
    assert o._collect() is None
    o.step()
    assert o.last_route() == "torch" and ps[0].dtype == torch.float64
    # the scalars of a replayed step need the kernel route
    with pytest.raises(RuntimeError, match="kernel route"):
        o.step(scalars_ready=True)
    assert o.prepare_scalars() is False
