"""The script that produced this directory's timing*.json: two builds of libpn2.so side by side on
the kernels only the streamed FPS and the raw-cloud downsampler run, interleaved in one process on
the same device buffers:

    python profiles/fps_host/bench_fps_ab.py <parent libpn2.so> <this libpn2.so> [--rounds 5] [--reps 3] [--out FILE]

(tools/bench_fps.py and tools/bench_downsample.py load one build per process; here both builds
share one process, one set of inputs and one set of output buffers, so neither placement nor the
other processes of a shared host separate them.)  Per case and round: parent, this, parent again
(the control), each `reps` back-to-back calls of the C entry point between two HIP events, after
one warm-up call per build whose outputs must be equal bit for bit.  One JSON line per case,
and with --out one document: every round's milliseconds per call, the medians, and the parent's
spread -- (max - min) / median over its 2 x rounds timings, control included -- the margin a
difference has to exceed to mean anything.  Needs a ROCm device."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"))
from pn2 import _lib  # noqa: E402

# streamed FPS (pn2_fps_ws_f32): (label, B, N, C, S); N = 0: the first multiple of 64 that needs the workspace
STREAM = [("stream_lds_16385", 32, 16385, 3, 512), ("stream_ws_first", 32, 0, 3, 256)]
# downsampler (pn2_fps_points): (label, B, N, C, dtype, number) -- tools/bench_downsample.py's batch shapes
POINTS = [("points_10k_f64", 64, 10000, 3, torch.float64, 1024), ("points_30k_f64", 64, 30000, 3, torch.float64, 1024),
          ("points_10k_f32", 64, 10000, 6, torch.float32, 1024)]


def bind(path):
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def stream_case(libs, B, N, C, S):
    if N == 0:
        N = 16384 + 64
        while libs[1].pn2_fps_workspace_bytes(B, N, C, S) == 0:
            N += 64
    g = torch.Generator().manual_seed(N)
    pts = (torch.rand(B, C, N, generator=g) * 2 - 1).cuda().permute(0, 2, 1)
    start = torch.randint(0, N, (B,), generator=g).cuda()
    cp = int(libs[1].pn2_packed_stride(C))
    need = int(libs[1].pn2_fps_workspace_bytes(B, N, C, S))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    o = [torch.empty(B, S, dtype=torch.int64, device="cuda"), torch.empty(B, S, C, device="cuda"),
         torch.empty(B, S, cp, device="cuda"), torch.empty(B, N, cp, device="cuda")]
    sb, sn, sc = pts.stride()

    def call(i):
        rc = libs[i].pn2_fps_ws_f32(pts.data_ptr(), B, N, C, sb, sn, sc, start.data_ptr(), S, o[0].data_ptr(),
                                    o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), ws.data_ptr() if need else None,
                                    need, None)
        assert rc == 0, libs[i].pn2_last_error()
    return call, o, {"B": B, "N": N, "C": C, "S": S, "distances": "workspace" if need else "lds"}


def points_case(libs, B, N, C, dtype, number):
    code = _lib.DTYPE_F64 if dtype == torch.float64 else _lib.DTYPE_F32
    g = torch.Generator().manual_seed(N + C)
    pts = (torch.rand(B, N, C, generator=g, dtype=dtype) * 2 - 1).cuda()
    table = torch.cat([torch.arange(B + 1) * N, torch.randint(0, N, (B,), generator=g)]).cuda()
    need = int(libs[1].pn2_fps_points_workspace_bytes(code, B * N, N))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    o = [torch.empty(B, number, dtype=torch.int64, device="cuda"), torch.empty(B, number, C, dtype=dtype, device="cuda")]

    def call(i):
        rc = libs[i].pn2_fps_points(pts.data_ptr(), code, B, table.data_ptr(), table.data_ptr() + 8 * (B + 1), B * N,
                                    N, C, C, number, o[0].data_ptr(), o[1].data_ptr(), ws.data_ptr() if need else None,
                                    need, None)
        assert rc == 0, libs[i].pn2_last_error()
    return call, o, {"B": B, "N": N, "C": C, "number": number, "dtype": str(dtype).split(".")[1],
                     "distances": "workspace" if need else "lds"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the rows as one JSON document to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fps_ab: needs a ROCm device")
    libs = [bind(os.path.abspath(a.parent)), bind(os.path.abspath(a.this))]
    rows = []
    for make, table in ((stream_case, STREAM), (points_case, POINTS)):
        for label, *shape in table:
            call, outs, info = make(libs, *shape)
            call(0)
            want = [x.clone() for x in outs]
            call(1)
            torch.cuda.synchronize()
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(want, outs)), label
            ms = ([], [], [])  # parent, this, parent again
            for _ in range(a.rounds):
                for j, i in enumerate((0, 1, 0)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        call(i)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[j].append(round(e0.elapsed_time(e1) / a.reps, 4))
            par = ms[0] + ms[2]
            med = [statistics.median(par), statistics.median(ms[1])]
            row = dict(info, case=label, parent_ms=ms[0], this_ms=ms[1], parent_control_ms=ms[2],
                       parent_median=med[0], this_median=med[1],
                       parent_spread=round((max(par) - min(par)) / med[0], 4),
                       this_over_parent=round(med[1] / med[0], 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        rec = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "rows": rows}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
