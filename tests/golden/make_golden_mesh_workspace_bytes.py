"""Records what the size queries of the six indexed-mesh units answer, as tests/golden/mesh_workspace_bytes.json:

    python triangle-splatting_amd/build.py && python tests/golden/make_golden_mesh_workspace_bytes.py

The queries (ts2d_weld_workspace_bytes of libts2d.so; tsq_, tss_, tsh_, tsf_ and tsw_workspace_bytes of libts_simplify.so, libts_smooth.so,
libts_holes.so, libts_manifold.so and libts_orient.so) are host code: they run without a GPU.  The record was taken from the commit before
the units' carving and scans were single-sourced (csrc/ts_mesh_common.h); tests/test_mesh_common_cpu.py holds every later build to it, byte
for byte.  Run it again only when a workspace is meant to change.

Counts: SIZES, the union of the tables of the units' test_size_query_is_monotone_in_both_counts tests, crossed with FIXED, once as the
vertex count and once as the face count.  Stored per query: by_v[i][j] = query(SIZES[j], FIXED[i]), by_f[i][j] = query(FIXED[i], SIZES[j]).
"""
import ctypes
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "triangle-splatting_amd")
SIZES = (0, 1, 2, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000)
FIXED = (0, 1000, 3000000)
QUERIES = {  # query -> its library, below the package
    "ts2d_weld_workspace_bytes": ("diff_triangle_rasterization_2D", "libts2d.so"),
    "tsq_workspace_bytes": ("diff_recon_hip", "libts_simplify.so"),
    "tss_workspace_bytes": ("diff_recon_hip", "libts_smooth.so"),
    "tsh_workspace_bytes": ("diff_recon_hip", "libts_holes.so"),
    "tsf_workspace_bytes": ("diff_recon_hip", "libts_manifold.so"),
    "tsw_workspace_bytes": ("diff_recon_hip", "libts_orient.so"),
}


def measure(package=PACKAGE):
    out = {"sizes": list(SIZES), "fixed": list(FIXED), "queries": {}}
    for name, where in QUERIES.items():
        query = getattr(ctypes.CDLL(os.path.join(package, *where)), name)
        query.restype, query.argtypes = ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]
        out["queries"][name] = {"by_v": [[query(n, fixed) for n in SIZES] for fixed in FIXED],
                                "by_f": [[query(fixed, n) for n in SIZES] for fixed in FIXED]}
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "mesh_workspace_bytes.json")
    text = json.dumps(measure(), indent=1)
    text = re.sub(r"\[\s+([\d,\s]+?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text)  # a row of numbers on one line
    with open(path, "w") as f:
        f.write(text + "\n")
    print("mesh_workspace_bytes.json:", os.path.getsize(path), "bytes")
