"""Generate tests/golden/downsample_<name>.npz by running the REFERENCE's numpy
farthest_point_sample(point_cloud, number) (provider.py:183-204).

Run only where /root/reference exists:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_downsample.py
provider.py imports open3d (absent here), so the function is compiled from its source text
alone, by the route make_goldens_augment.py takes: read only, nothing copied into the
repository -- the fixtures are data.

The reference carries the function in several files; the copies listed in COPIES are first
asserted to be the same function: equal ASTs once the docstring and the default of `number` are
dropped and every name is replaced by its order of first appearance (the ModelNet loader calls
its arguments (point, npoint) and the column count D).

Each file: seed (np.random.seed), cloud ([N, C] float64 or float32), number, rows (the function's
result), idx (int64 [number]: the rows it picked -- read off a second run, under the same seed,
of the cloud with one more column holding 0..N-1, which the function carries along but does not
measure), next_draw (one np.random.random() taken after the call, which pins how much of the
generator it consumed) and prop, the name in downsample_ref.PROPERTIES of what the case is there
for.  The seeds are searched, on the CPU, until that property holds."""
import ast
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
COPIES = ("provider.py", "data_utils/ModelDataLoader.py", "data_utils/ModelNetDataLoader.py",
          "point_collect/transformer.py", "colledt_data_structure/transformer.py",
          "data_build/Cube.py", "data_build/Cube_cylinder.py", "data_build/Cylinder.py",
          "data_build/Double_cube.py", "data_build/Double_cylinder.py", "data_build/H_structure.py")

import numpy as np  # noqa: E402

import downsample_ref  # noqa: E402


def _function(path):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    found = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "farthest_point_sample"]
    assert len(found) == 1, path
    return found[0]


def _canonical(fn):
    """The function's AST dump without docstring and defaults, names by first appearance."""
    fn = ast.parse(ast.unparse(fn)).body[0]
    if isinstance(fn.body[0], ast.Expr) and isinstance(getattr(fn.body[0], "value", None), ast.Constant):
        fn.body = fn.body[1:]
    fn.args.defaults = []
    names = {}
    for node in ast.walk(fn):
        if isinstance(node, ast.arg):
            node.arg = names.setdefault(node.arg, "v%d" % len(names))
    for node in ast.walk(fn):
        if isinstance(node, ast.Name) and node.id != "np" and node.id != "range":
            node.id = names.setdefault(node.id, "v%d" % len(names))
    return ast.dump(fn)


def reference_function():
    dumps = {p: _canonical(_function(p)) for p in COPIES}
    first = dumps[COPIES[0]]
    for p, d in dumps.items():
        assert d == first, "%s differs from %s" % (p, COPIES[0])
    ns = {"np": np}
    exec(compile(ast.Module(body=[_function(COPIES[0])], type_ignores=[]), "provider.py", "exec"), ns)
    return ns["farthest_point_sample"]


# ------------------------------------------------------------------------------- the clouds
def _uniform(rs, N, C, dtype):
    return rs.uniform(-1.0, 1.0, (N, C)).astype(dtype)


def _lattice(rs, N, C, dtype):
    """Grid points with coordinates that are multiples of 1/8, as data_build's shapes are laid
    out, in shuffled order: exact distance ties everywhere."""
    side = int(round(N ** (1.0 / 3)))
    g = np.arange(side) / 8.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = pts[rs.permutation(len(pts))]
    extra = rs.uniform(-1.0, 1.0, (len(pts), C - 3))
    return np.concatenate([pts, extra], 1).astype(dtype)


def _duplicated(rs, N, C, dtype):
    """Every row present twice, at unrelated positions."""
    half = _uniform(rs, N // 2, C, dtype)
    both = np.concatenate([half, half], 0)
    return both[rs.permutation(len(both))]


def _scaled(rs, N, C, dtype):
    """Well separated points scaled by 1e6: every pairwise squared distance is far above 1e10."""
    pts = _lattice(rs, N, C, dtype)
    pts[:, :3] *= 8.0e6
    return pts


def _sphere(rs, N, C, dtype):
    """Points on the unit sphere, as a normalised shape's shell: many near-equal distances, which
    is where a different rounding changes the argmax."""
    p = rs.normal(size=(N, C))
    p[:, :3] /= np.linalg.norm(p[:, :3], axis=1, keepdims=True)
    return p.astype(dtype)


def _decimal_grid(rs, N, C, dtype):
    """Grid points at multiples of 0.1, shuffled: the symmetric distances that are equal on paper
    differ in their last bits, by the rounding of each inexact square -- the argmax among them is
    what a contracted (fused) square changes, even in float64."""
    pts = _lattice(rs, N, C, np.float64)
    pts[:, :3] = np.round(pts[:, :3] * 8.0) * 0.1
    return pts.astype(dtype)


# name -> (cloud builder, N, C, dtype, number, property)
CASES = {
    "one": (_uniform, 1, 3, np.float64, 4, "repeat"),
    "five": (_uniform, 5, 3, np.float64, 9, "repeat"),
    "lattice": (_lattice, 216, 3, np.float64, 64, "ties"),
    "lattice32": (_lattice, 343, 3, np.float32, 64, "ties"),
    "dup": (_duplicated, 300, 3, np.float64, 48, "ties"),
    "wide32": (_sphere, 1500, 3, np.float32, 128, "wide"),
    "fma32": (_sphere, 1500, 3, np.float32, 128, "fma"),
    "fma64": (_decimal_grid, 216, 3, np.float64, 32, "fma"),
    "far": (_scaled, 125, 3, np.float64, 32, "far"),
    "c4": (_uniform, 257, 4, np.float64, 40, "columns"),
    "c6": (_sphere, 1030, 6, np.float32, 64, "columns"),
    "modelnet": (_sphere, 2048, 6, np.float32, 1024, "plain"),
    "camera": (_uniform, 2000, 3, np.float64, 1024, "plain"),
}


def main():
    ref = reference_function()
    seen = set()
    for k, (name, (build, N, C, dtype, number, prop)) in enumerate(CASES.items()):
        seed = 2000 + 100000 * k
        while True:
            cloud = build(np.random.RandomState(seed), N, C, dtype)
            assert cloud.dtype == dtype and cloud.shape[1] == C
            tagged = np.concatenate([cloud, np.arange(len(cloud), dtype=dtype)[:, None]], 1)
            np.random.seed(seed)
            idx = ref(tagged, number)[:, -1].astype(np.int64)
            if downsample_ref.PROPERTIES[prop](cloud, number, idx):
                break
            seed += 1
        np.random.seed(seed)
        rows = ref(cloud, number)
        next_draw = np.random.random()
        assert rows.dtype == dtype and np.array_equal(rows, cloud[idx])
        assert len(cloud) < 2 ** 24  # the index column is exact in float32
        seen.add(prop)
        path = os.path.join(HERE, "downsample_%s.npz" % name)
        np.savez_compressed(path, seed=np.array(seed), cloud=cloud, number=np.array(number), idx=idx,
                            rows=rows, next_draw=np.array(next_draw), prop=np.array(prop))
        print("downsample", name, "seed", seed, cloud.shape, cloud.dtype, "number", number, prop,
              os.path.getsize(path), "bytes")
    assert seen == set(downsample_ref.PROPERTIES), seen


if __name__ == "__main__":
    main()
