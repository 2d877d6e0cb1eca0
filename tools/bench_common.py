"""What the route-against-route bench tools share (bench_fc_train.py, bench_fc_rows.py,
bench_loss.py, bench_train_gemm.py, bench_group_backward.py): HIP events around `reps`
back-to-back calls, routes interleaved within each of `rounds` rounds after `warmup` calls,
median (min, max) of the rounds."""
import statistics

import torch

from pn2 import tuning

# the keys under which a PointNet++ head's train step has no order-dependent sum up to 64 rows
REPRO = {"train_gemm": 1, "group_backward": 1, "train_head": 1}


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(runs, a):
    """runs: name -> (tuning keys, fn).  -> name -> the rounds' ms per call."""
    for keys, fn in runs.values():
        with tuning.override(**keys):
            for _ in range(a.warmup):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (keys, fn) in runs.items():
            with tuning.override(**keys):
                ms[k].append(timed(fn, a.reps))
    return ms


def two_routes(runs, a):
    """runs: two routes, name -> (tuning keys, fn) -> their summaries and
    ratio_<first>_over_<second> of the medians (> 1: the second is faster)."""
    first, second = runs
    ms = interleaved(runs, a)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"ms": {k: summary(v) for k, v in ms.items()},
            "ratio_%s_over_%s" % (first, second): round(med[first] / med[second], 3)}
