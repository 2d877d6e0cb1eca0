"""torch.optim.Adam and torch.optim.SGD whose step is ONE HIP launch over every parameter
(csrc/optim.hip, include/pn2.h pn2_adam_step_f32 / pn2_sgd_step_f32).

The reference's train scripts step ``torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-08,
weight_decay=args.decay_rate)`` (or ``SGD(lr=0.01, momentum=0.9)``) after every batch, with
``StepLR(step_size=20, gamma=0.7)`` on top (train_classification.py:88-101, 128).  ``pn2.optim.Adam``
and ``pn2.optim.SGD`` are subclasses with the same constructors, ``param_groups`` and state layout
(``state[p]['step']`` a CPU float32 tensor, ``exp_avg`` / ``exp_avg_sq`` / ``momentum_buffer``),
so state dicts move both ways between them and torch's classes, and schedulers drive
``param_groups[i]['lr']`` as before.

Which route a ``step()`` takes (``last_route()`` tells: "kernel" or "torch"):
  the kernel, when every parameter that has a gradient is a dense, contiguous float32 device
  tensor on one device with a gradient (and state) of the same layout, and the options are the
  ones the kernel implements -- Adam without amsgrad / maximize / capturable / differentiable /
  fused / decoupled_weight_decay, SGD with momentum >= 0 and without nesterov / maximize / fused /
  differentiable; float options, not tensors;
  otherwise ``super().step()`` for the whole call, unchanged (CPU tensors included).
Parameters whose ``.grad`` is None are skipped and their ``step`` does not advance, as in torch.

The step's scalars (step size with bias correction, betas, eps, weight decay, ...) are computed
on the host in Python floats with torch's own expressions, rounded to float32 once, and written
to DEVICE memory before each launch -- they are never kernel arguments.  So a launch captured
into a graph replays with the values of the step being replayed:

    opt.prepare_scalars()            # outside the graph: advances `step`, uploads the scalars
    graph.replay()                   # holds opt.step(scalars_ready=True)

``prepare_scalars()`` works on the parameters that have a gradient now; when none has one
(``zero_grad(set_to_none=True)`` before a backward that is about to be captured) on those of the
last launch.  The descriptor table (pointers, counts) is rebuilt only when a parameter's or a
gradient's address changes, and uploaded into the same device buffer outside any capture: a
launch captured while the table changed has its upload done by ``upload_table()`` or by the
next ``prepare_scalars()``, before its first replay.

State tensors are looked up when the table is built.  ``load_state_dict`` rebuilds it; code that
replaces ``exp_avg`` and the like by hand calls ``invalidate()``.
"""
import numpy as np
import torch
from torch.optim.optimizer import _get_scalar_dtype

from . import _lib

_RING = 8  # pinned scalar buffers in flight before the host waits for the oldest copy


def _dense_f32(t, device):
    return (t.dtype == torch.float32 and t.device == device and t.layout == torch.strided and t.is_contiguous()
            and not t.is_complex())


class _KernelStep:
    """The table / scalar / launch machinery shared by Adam and SGD (a mixin in front of the
    torch class)."""

    _ENTRY = None  # "pn2_adam_step_f32" / "pn2_sgd_step_f32"

    # ---- per-class pieces
    def _options_ok(self, group):
        raise NotImplementedError

    def _advance(self, gi, group, p):
        """Advance the tensor's step (creating lazily what torch creates) -> the variant of its
        scalar block: tensors of one group with one variant share a block."""
        raise NotImplementedError

    def _state_tensors(self, gi, group, p, g):
        """(m, v) for the descriptor table."""
        raise NotImplementedError

    def _block(self, group, variant):
        raise NotImplementedError

    # ---- bookkeeping
    def _k(self):
        k = self.__dict__.get("_pn2k")
        if k is None:
            k = self.__dict__["_pn2k"] = {"route": None, "key": None, "items": None, "pending": False,
                                          "ring": None, "slot": 0, "prepared": None, "uploads": 0}
        return k

    def last_route(self):
        """"kernel" or "torch": the route of the last step() (None before the first)."""
        return self._k()["route"]

    def table_uploads(self):
        """How many times the descriptor table was uploaded (it follows moved gradients)."""
        return self._k()["uploads"]

    def invalidate(self):
        """Forget the descriptor table (state tensors were replaced by hand)."""
        k = self._k()
        k["key"] = None
        k["prepared"] = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.invalidate()

    def _collect(self):
        """[(group index, p, grad)] of the parameters with a gradient; None when one of them, or
        an option, is outside what the kernel implements."""
        items = []
        device = None
        for gi, group in enumerate(self.param_groups):
            ok = None
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if ok is None:
                    ok = self._options_ok(group)
                if device is None:
                    device = p.device
                if not ok or device.type != "cuda" or not _dense_f32(p, device) or not _dense_f32(g, device) \
                        or g.shape != p.shape:
                    return None
                items.append((gi, p, g))
        return items

    # ---- the host half
    def prepare_scalars(self):
        """Advance `step`, compute this step's scalar blocks and upload them on the current
        stream (and a table upload a capture left pending).  Returns False when the kernel route
        does not apply (nothing is done then)."""
        items = self._collect()
        if items is not None and not items:
            last = self._k()["items"]
            items = [(gi, p, None) for gi, p, _ in last] if last else items
        if not items:
            return False
        self._prepare(items)
        return True

    def _prepare(self, items):
        k = self._k()
        if k["pending"]:
            self.upload_table()
        blocks, index, which = [], {}, []
        groups = self.param_groups
        for gi, p, g in items:
            variant = self._advance(gi, groups[gi], p)
            key = (gi, variant)
            b = index.get(key)
            if b is None:
                b = index[key] = len(blocks)
                blocks.append(self._block(groups[gi], variant))
            which.append(b)
        device = items[0][1].device
        ring = k["ring"]
        cap = len(items)
        if ring is None or ring["cap"] < cap or ring["device"] != device:
            ns = int(_lib.load().pn2_optim_scalars())
            ring = k["ring"] = {
                "cap": cap, "ns": ns, "device": device,
                "host": [torch.zeros(cap * ns, dtype=torch.float32).pin_memory() for _ in range(_RING)],
                "events": [None] * _RING,
                "dev": torch.zeros(cap * ns, dtype=torch.float32, device=device),
            }
            ring["np"] = [h.numpy() for h in ring["host"]]
            k["key"] = None  # the scalar buffer moved: the launch arguments change
        s = k["slot"] = (k["slot"] + 1) % _RING
        ev = ring["events"][s]
        if ev is not None:
            ev.synchronize()  # the copy that last read this pinned buffer is done
        n = len(blocks) * ring["ns"]
        ring["np"][s][:n] = np.asarray(blocks, dtype=np.float64).reshape(-1)  # one rounding to float32
        ring["dev"][:n].copy_(ring["host"][s][:n], non_blocking=True)
        if ev is None:
            ev = ring["events"][s] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        k["prepared"] = ([id(p) for _, p, _ in items], which, len(blocks))

    # ---- the launch
    def upload_table(self):
        """Upload a descriptor table that changed during a stream capture (the capture records
        the launch only; the table must be on the device before the first replay)."""
        k = self._k()
        if k["pending"]:
            # pinned here, outside any capture; torch's host allocator keeps a pinned block until
            # the copy that reads it is done
            k["dev_tab"].copy_(k["host_tab"].pin_memory(), non_blocking=True)
            k["dev_jobs"].copy_(k["host_jobs"].pin_memory(), non_blocking=True)
            k["pending"] = False
            k["uploads"] += 1

    def _launch(self, items):
        k = self._k()
        ids, which, nblocks = k["prepared"]
        if ids != [id(p) for _, p, _ in items]:
            raise RuntimeError("pn2.optim: step(scalars_ready=True) for other parameters than "
                               "prepare_scalars() prepared")
        key = (tuple(which), tuple([x for _, p, g in items for x in (p.data_ptr(), g.data_ptr())]))
        L = _lib.load()
        device = items[0][1].device
        if key != k["key"]:
            groups = self.param_groups
            rows = []
            for (gi, p, g), b in zip(items, which):
                m, v = self._state_tensors(gi, groups[gi], p, g)[:2]
                for t in (m, v):
                    if t is not None and (not _dense_f32(t, device) or t.shape != p.shape):
                        raise RuntimeError("pn2.optim: optimizer state of another layout than its parameter")
                rows.append((p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(),
                             0 if v is None else v.data_ptr(), p.numel(), b))
            chunk = int(L.pn2_optim_chunk())
            tab = np.asarray(rows, dtype=np.int64)
            nch = (tab[:, 4] + chunk - 1) // chunk
            jobs = np.empty((int(nch.sum()), 2), dtype=np.int32)
            jobs[:, 0] = np.repeat(np.arange(len(rows), dtype=np.int32), nch)
            jobs[:, 1] = np.concatenate([np.arange(c, dtype=np.int32) for c in nch]) if len(rows) else 0
            # the host copy is what the entry's argument check reads; the device buffers are
            # reused while the sizes hold, so a captured launch keeps its arguments
            k["host_tab"] = torch.from_numpy(tab)
            k["host_jobs"] = torch.from_numpy(jobs)
            old = k.get("dev_tab")
            if old is None or old.shape != k["host_tab"].shape or old.device != device \
                    or k["dev_jobs"].shape != k["host_jobs"].shape:
                k["dev_tab"] = torch.empty(tab.shape, dtype=torch.int64, device=device)
                k["dev_jobs"] = torch.empty(jobs.shape, dtype=torch.int32, device=device)
            k["pending"] = True
            if not torch.cuda.is_current_stream_capturing():
                self.upload_table()
            k["key"] = key
            k["items"] = [(gi, p, None) for gi, p, _ in items]  # no hold on the gradients
        tab, jobs = k["host_tab"], k["dev_jobs"]
        rc = getattr(L, self._ENTRY)(tab.data_ptr(), k["dev_tab"].data_ptr(), tab.shape[0], jobs.data_ptr(),
                                     jobs.shape[0], k["ring"]["dev"].data_ptr(), nblocks,
                                     _lib.stream_ptr(device))
        _lib.check(rc, self._ENTRY)

    def _kernel_step(self, closure, scalars_ready):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        k = self._k()
        items = self._collect()
        if items is None:
            if scalars_ready:
                raise RuntimeError("pn2.optim: step(scalars_ready=True) needs the kernel route (dense "
                                   "contiguous float32 device tensors, supported options)")
            k["route"] = "torch"
            super().step()
            return loss
        k["route"] = "kernel"
        if not items:
            return loss
        if not scalars_ready:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("pn2.optim: inside a stream capture call prepare_scalars() before the "
                                   "capture and step(scalars_ready=True) in it")
            self._prepare(items)
        elif k["prepared"] is None:
            raise RuntimeError("pn2.optim: step(scalars_ready=True) before prepare_scalars()")
        with torch.no_grad():
            self._launch(items)
        return loss


class Adam(_KernelStep, torch.optim.Adam):
    """torch.optim.Adam with the update of every parameter in one HIP launch (module docstring)."""

    _ENTRY = "pn2_adam_step_f32"

    def _options_ok(self, group):
        if (group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"]
                or group["fused"] or group.get("decoupled_weight_decay", False)):
            return False
        b1, b2 = group["betas"]
        return all(isinstance(x, (int, float)) for x in (group["lr"], b1, b2, group["eps"], group["weight_decay"]))

    def _state(self, p):
        state = self.state[p]
        if len(state) == 0:  # torch's lazy initialisation, Adam._init_group
            state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _advance(self, gi, group, p):
        step_t = self._state(p)["step"]
        step_t += 1
        return step_t.item()

    def _state_tensors(self, gi, group, p, g):
        state = self._state(p)
        return state["exp_avg"], state["exp_avg_sq"]

    def _block(self, group, step):
        # torch's _single_tensor_adam, in Python floats
        beta1, beta2 = group["betas"]
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = group["lr"] / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        return (-step_size, bias_correction2_sqrt, 1 - beta1, beta2, 1 - beta2, group["eps"],
                group["weight_decay"], 0.0)

    def step(self, closure=None, scalars_ready=False):
        return self._kernel_step(closure, scalars_ready)


class SGD(_KernelStep, torch.optim.SGD):
    """torch.optim.SGD (momentum, dampening, weight decay) with the update of every parameter in
    one HIP launch (module docstring)."""

    _ENTRY = "pn2_sgd_step_f32"

    def _options_ok(self, group):
        if (group["nesterov"] or group["maximize"] or group.get("fused") or group.get("differentiable")
                or group["momentum"] < 0):
            return False
        return all(isinstance(group[x], (int, float)) for x in ("lr", "momentum", "dampening", "weight_decay"))

    def _advance(self, gi, group, p):
        # the variant of the scalar block: whether this step creates the momentum buffer
        if group["momentum"] == 0:
            return 0.0
        state = self.state[p]
        if state.get("momentum_buffer") is None:
            # torch: buf = clone(grad) on the first step; the kernel writes it (first != 0)
            state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
            self._k()["key"] = None
            return 1.0
        return 0.0

    def _state_tensors(self, gi, group, p, g):
        if group["momentum"] == 0:
            return None, None
        return self.state[p]["momentum_buffer"], None

    def _block(self, group, first):
        return (group["lr"], group["momentum"], 1 - group["dampening"], group["weight_decay"], first, 0.0, 0.0, 0.0)

    def step(self, closure=None, scalars_ready=False):
        return self._kernel_step(closure, scalars_ready)
