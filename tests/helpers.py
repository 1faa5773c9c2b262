"""Shared helpers for the parity tests: run one scene through the CPU oracle and through the HIP path
(via the drop-in Python package, i.e. through the C ABI), and compare."""
from __future__ import annotations

import os

import numpy as np

import synthetic
from oracle import ts2d_oracle as O


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = np.linalg.norm((a - b).ravel())
    n = np.linalg.norm(b.ravel())
    return d / n if n > 0 else d


def oracle_forward(s, rich_info=True, back_culling=False, use_feature=False, variant=2):
    shs = None if use_feature else s["shs"]
    feature = s["feature"] if use_feature else None
    n, img, radii, depth, normal, csum, cmax, st = O.rasterize_triangles(
        s["image_width"], s["image_height"], s["tanfovx"], s["tanfovy"], s["viewmatrix"], s["projmatrix"], s["campos"],
        s["sh_degree"], s["gamma"], s["scale_modifier"], s["background_depth"], s["background"], s["vertex"], shs,
        feature, s["opacity"], back_culling, rich_info, variant=variant)
    return dict(num_rendered=n, out_feature=img, radii=radii, depth=depth, normal=normal, contrib_sum=csum,
                contrib_max=cmax, state=st)


def oracle_backward(s, fwd, rich_info=True, use_feature=False):
    shs = None if use_feature else s["shs"]
    feature = s["feature"] if use_feature else None
    dv, dc, dsh, df, dop = O.rasterize_triangles_backward(
        s["tanfovx"], s["tanfovy"], s["viewmatrix"], s["projmatrix"], s["campos"], s["sh_degree"], s["gamma"],
        s["scale_modifier"], s["background_depth"], s["background"], s["vertex"], shs, feature, s["opacity"],
        fwd["radii"], fwd["state"], s["dL_dout_feature"], s.get("dL_dout_depth"), s.get("dL_dout_normal"), rich_info)
    return dict(dL_dvertex=dv, dL_dcenter2D=dc, dL_dshs=dsh, dL_dfeature=df, dL_dopacity=dop)


def hip_settings(s, rich_info=True, back_culling=False, debug=False, device="cuda"):
    import torch
    from diff_triangle_rasterization_2D import TriangleRasterizationSettings

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return TriangleRasterizationSettings(
        image_width=s["image_width"], image_height=s["image_height"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
        viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]), campos=t(s["campos"]), sh_degree=s["sh_degree"],
        gamma=s["gamma"], scale_modifier=s["scale_modifier"], background_depth=s["background_depth"],
        background=t(s["background"]), back_culling=back_culling, rich_info=rich_info, debug=debug)


def hip_forward_backward(s, rich_info=True, back_culling=False, use_feature=False, backward=True, device="cuda", debug=False,
                         variant=2, depth_normal_grads="given"):
    """Runs the HIP path through the drop-in autograd module.  Returns numpy outputs + grads + raw state.
    depth_normal_grads: "given" = the scene's dL_dout_depth / dL_dout_normal; "zeros" = two images of zeros handed in; "none" = the loss reads
    the colours only (autograd hands the module None for depth and normal)."""
    import torch
    if variant == 3:
        from diff_triangle_rasterization_3D import TriangleRasterizer
    else:
        from diff_triangle_rasterization_2D import TriangleRasterizer

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    rs = hip_settings(s, rich_info, back_culling, debug, device)
    vertex = t(s["vertex"]).requires_grad_(True)
    opacity = t(s["opacity"]).requires_grad_(True)
    center2D = torch.zeros((vertex.shape[0], 2), device=device, requires_grad=True)
    shs = feature = None
    if use_feature:
        feature = t(s["feature"]).requires_grad_(True)
    else:
        shs = t(s["shs"]).requires_grad_(True)
    out = TriangleRasterizer(rs)(vertex, center2D, opacity, shs=shs, feature=feature)
    res = dict(out_feature=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy())
    if rich_info:
        res.update(depth=out[2].detach().cpu().numpy(), normal=out[3].detach().cpu().numpy(),
                   contrib_sum=out[4].cpu().numpy(), contrib_max=out[5].cpu().numpy())
    node = out[0].grad_fn
    res["num_rendered"] = node.num_rendered
    saved = node.saved_tensors
    res["buffers"] = saved[5:8]
    if backward:
        loss = (out[0] * t(s["dL_dout_feature"])).sum()
        if rich_info and depth_normal_grads != "none":
            k = 0.0 if depth_normal_grads == "zeros" else 1.0
            loss = loss + (out[2] * (k * t(s["dL_dout_depth"]))).sum() + (out[3] * (k * t(s["dL_dout_normal"]))).sum()
        loss.backward()
        res.update(dL_dvertex=vertex.grad.cpu().numpy(), dL_dcenter2D=center2D.grad.cpu().numpy(),
                   dL_dopacity=opacity.grad.cpu().numpy())
        if use_feature:
            res["dL_dfeature"] = feature.grad.cpu().numpy()
        else:
            res["dL_dshs"] = shs.grad.cpu().numpy()
    return res


# ---- private-state reader: tools/bin/libts2d_lab.so (csrc/ts2d_lab.h) ---------------------------------------------------------
# The product library exports no diagnostics.  The lab library contains the product's objects (same layout code), so its reader
# decodes the state buffers of a forward that the PRODUCT library ran in this process.
LAB_LIB = os.environ.get("TS2D_LAB_LIBRARY_PATH") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin", "libts2d_lab.so")  # the override: a variant build's lab library (build.py --variant TAG --lab)
_lab = None


def lab_library():
    global _lab
    if _lab is None:
        import ctypes as C
        if not os.path.exists(LAB_LIB):
            raise RuntimeError(f"{LAB_LIB} not found: build it with `python triangle-splatting_amd/build.py --lab`")
        # the package first: the lab library carries the soname libts2d.so too, and the extension binds the first library of that name loaded
        from diff_triangle_rasterization_2D import _C as product
        from diff_triangle_rasterization_2D import _abi
        L = _abi.bind(C.CDLL(LAB_LIB))  # the product's signatures and those of csrc/ts2d_lab.h
        # same layout code as the product library?  (a lab library left over from before a change of csrc/ts2d_common.h decodes other offsets)
        for f, args in (("ts2d_geometry_state_bytes", (C.c_int32(12345),)), ("ts2d_binning_state_bytes", (C.c_int64(54321), C.c_int32(640), C.c_int32(480))),
                        ("ts2d_binning_state_bytes", (C.c_int64(7654321), C.c_int32(1920), C.c_int32(1080))), ("ts2d_image_state_bytes", (C.c_int32(640), C.c_int32(480)))):
            mine, theirs = getattr(L, f), getattr(product._lib, f)
            if mine(*args) != theirs(*args):
                raise RuntimeError(f"{LAB_LIB} is stale ({f} differs from the product library's): rebuild it with `python triangle-splatting_amd/build.py --lab`")
        _lab = L
    return _lab


def _field_spec():
    import torch
    return {
        "v_2D": (0, torch.float32, lambda P, N, T, HW: (P, 6)), "area2": (1, torch.float32, lambda P, N, T, HW: (P,)),
        "normal_view": (2, torch.float32, lambda P, N, T, HW: (P, 3)), "v_depth": (3, torch.float32, lambda P, N, T, HW: (P, 3)),
        "depth": (4, torch.float32, lambda P, N, T, HW: (P,)), "rgb": (5, torch.float32, lambda P, N, T, HW: (P, 3)),
        "clamped": (6, torch.uint8, lambda P, N, T, HW: (P,)), "point_offsets": (7, torch.int32, lambda P, N, T, HW: (P,)),
        "tiles_touched": (8, torch.int32, lambda P, N, T, HW: (P,)), "rect": (9, torch.int32, lambda P, N, T, HW: (P, 4)),
        "keys": (10, torch.int64, lambda P, N, T, HW: (N,)), "vals": (11, torch.int32, lambda P, N, T, HW: (N,)),
        "ranges": (12, torch.int32, lambda P, N, T, HW: (T, 2)), "n_contrib": (13, torch.int32, lambda P, N, T, HW: HW),
        "final_T": (14, torch.float32, lambda P, N, T, HW: HW), "tile_unsorted": (15, torch.int32, lambda P, N, T, HW: (N,)),
        "vals_unsorted": (16, torch.int32, lambda P, N, T, HW: (N,)), "depth_perm": (17, torch.int32, lambda P, N, T, HW: (P,)),
        "records": (18, torch.float32, lambda P, N, T, HW: (P, 16)),
    }


def debug_read_state(name, P, num_rendered, W, H, geometryBuffer, binningBuffer, imageBuffer):
    """Copies one private state array to a CPU tensor (ts2d_debug_read_state of the lab library, csrc/ts2d_lab.h)."""
    import ctypes as C
    import torch
    L = lab_library()
    field, dtype, shape = _field_spec()[name]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    out = torch.empty(shape(P, num_rendered, T, (H, W)), dtype=dtype)
    from diff_triangle_rasterization_2D._abi import _State as State
    ptr = lambda t: t.data_ptr() if t.numel() else None
    st = State(ptr(geometryBuffer), geometryBuffer.numel(), ptr(binningBuffer), binningBuffer.numel(), ptr(imageBuffer), imageBuffer.numel())
    with torch.cuda.device(geometryBuffer.device):
        rc = L.ts2d_debug_read_state(C.byref(st), P, num_rendered, W, H, field, out.data_ptr(), out.numel() * out.element_size(),
                                     torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"debug_read_state: {L.ts2d_last_error().decode()} (ts2d error {rc})")
    return out


def hip_state(res, s, name):
    g, b, im = res["buffers"]
    P = s["vertex"].shape[0]
    a = debug_read_state(name, P, res["num_rendered"], s["image_width"], s["image_height"], g, b, im).numpy()
    if name in ("vals", "vals_unsorted"):
        a = a & 0x0FFFFFFF  # triangle ids; the four bits above TS_ID_BITS hold the instance's quadrant mask (csrc/ts2d_support.h)
    return a


def grazing_mask(of, cos_limit):
    """3D variant: triangles whose plane is seen within acos(cos_limit) of edge-on (from the oracle's view-space state).
    There depth = v1.n / p_ray.n (R3D forward.cu:243-244) loses a factor 1 / cos of precision in ANY fp32 evaluation."""
    st = of["state"]
    c = (st.field("v1_view").astype(np.float64) + st.field("v2_view") + st.field("v3_view")) / 3.0
    n = st.field("normal_view").astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cosv = np.abs((c * n).sum(1)) / (np.linalg.norm(c, axis=1) * np.linalg.norm(n, axis=1))
    return np.nan_to_num(cosv, nan=1.0) < cos_limit


def robust_rel_l2(hip, ora, budget, exclude=None, ref=None, dropped_bound=None):
    """rel-L2 over triangles (or pixels) after setting aside `exclude` (bool mask) and the `budget` largest per-row errors.
    The error is measured against the norm of the KEPT rows of `ora` (or `ref` when given).  The rows that were set aside
    must still be sane: finite, and -- when `dropped_bound` is given -- each within dropped_bound x max(its own reference
    magnitude, the median magnitude of the non-zero rows), so that a garbage row cannot hide inside the budget."""
    P = hip.shape[0]
    h = hip.astype(np.float64).reshape(P, -1)
    o = ora.astype(np.float64).reshape(P, -1)
    assert np.isfinite(h).all(), "non-finite values in the compared output"
    err = np.linalg.norm(h - o, axis=1)
    mag = np.linalg.norm(o, axis=1)
    keep = np.ones(P, bool)
    if exclude is not None:
        keep &= ~exclude
    if budget > 0:
        order = np.argsort(np.where(keep, err, -1.0))
        keep[order[P - budget:]] = False
    if dropped_bound is not None and (~keep).any():
        nz = mag[mag > 0]
        floor = float(np.median(nz)) if nz.size else 0.0
        bad = err[~keep] > dropped_bound * np.maximum(mag[~keep], floor)
        assert not bad.any(), f"{int(bad.sum())} set-aside rows are off by more than {dropped_bound}x their own scale"
    d = np.sqrt((err[keep] ** 2).sum())
    n = np.sqrt((mag[keep] ** 2).sum()) if ref is None else ref
    return d / n if n > 0 else d


# ---- THE criterion for the floating-point outputs of the 3D variant ---------------------------------------------------------
# The 3D rasterizer's per-pixel ray / plane arithmetic (R3D forward.cu:238-256) is ill-conditioned: depth = v1.n / p_ray.n cancels for
# triangles seen edge-on and one ulp of the depth moves the barycentrics by ~depth / edge ulps, so WHICH products a compiler fuses into
# FMAs decides arg-min ties and whole gradients of grazing triangles.  No outlier budget can be justified for
# that; the yardstick is the reference's distance to ITSELF: its own sources built three ways (oracle/build_ref.py),
#     _ref3d_C         hipcc defaults (-ffp-contract=fast + SLP vectorizer),
#     _ref3d_scalar_C  -fno-slp-vectorize (every a*b+c fuses; what the product's kernels also do),
#     _ref3d_nofma_C   -ffp-contract=off (the CPU oracle reproduces this build to 1e-6).
# Every output of the product, WITHOUT any budget or mask, must be (i) at least as close to one build as the builds typically are to
# each other (the median of their three pairwise distances: two builds can coincide by accident, e.g. at gamma = 50 the default and
# the contraction-free build sit 4e-4 apart while the third is 3e-3 from both) and (ii) no further from any build than the two most
# distant builds are from each other (x 1.25) -- or meet the north-star bar outright where the builds agree better than that.
R3D_BUILDS = ("_ref3d_C", "_ref3d_scalar_C", "_ref3d_nofma_C")
R3D_BARS = {"out_feature": 1e-4, "depth": 3e-4, "normal": 3e-4, "contrib_sum": 3e-4, "contrib_max": 3e-4,
            "dL_dshs": 1e-3, "dL_dfeature": 1e-3, "dL_dopacity": 1e-3, "dL_dvertex": 1e-3, "dL_dcenter2D": 1e-3}


_ref_server = None


def _ref_request(line, timeout=600):
    """One request to the reference-kernel server process (tests/ref_worker.py --serve); starts it on demand.  Returns the answer
    line, or None when the process died (a signal inside the reference's kernels): the next request starts a fresh one."""
    global _ref_server
    import os
    import select
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for attempt in range(2):
        if _ref_server is None or _ref_server.poll() is not None:
            _ref_server = subprocess.Popen([sys.executable, os.path.join(here, "ref_worker.py"), "--serve"], stdin=subprocess.PIPE,
                                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, bufsize=1)
            ready, _, _ = select.select([_ref_server.stdout], [], [], 300)
            if not ready or _ref_server.stdout.readline().strip() != "ready":
                _ref_server.kill()
                _ref_server = None
                raise RuntimeError("the reference-kernel server did not start")
        try:
            _ref_server.stdin.write(line + "\n")
            _ref_server.stdin.flush()
        except BrokenPipeError:
            _ref_server = None
            _sweep_device_caches()
            continue
        ready, _, _ = select.select([_ref_server.stdout], [], [], timeout)
        ans = _ref_server.stdout.readline().strip() if ready else ""
        if ans:
            return ans
        _ref_server.kill()
        _ref_server.wait()
        _ref_server = None
        _sweep_device_caches()
        return None
    return None


def _sweep_device_caches():
    """Called after the reference-kernel server died.  It dies of GPU memory-access faults inside the reference's kernels, and on this platform
    a process that faults leaves the SURVIVING processes on the device with stale cache lines: the next large launch of this process can then
    read memory as it was before its own memset / atomics (whole 128-byte lines of the backward's gradient records; measured in round 4 with
    a faulting neighbour that ran none of the reference's code: 6 of 8 runs wrong, none without a faulting neighbour, none with this sweep --
    profiles/r04_neighbour_fault.txt).  Writing and re-reading 2 GiB pushes every line of the
    eight L2s and of the memory-side cache out while nothing of this process is live."""
    import torch
    if not torch.cuda.is_available():
        return
    x = torch.empty(2 << 30, dtype=torch.uint8, device="cuda")
    x.fill_(1)
    x.add_(1)
    torch.cuda.synchronize()
    del x
    torch.cuda.empty_cache()


def ref3d_builds(s, rich=True, back=False, use_feature=False, fuzz_seed=None):
    """{build: outputs} of the reference's 3D extension built three ways on the scene `s`, or None when oracle/_ref is absent, the
    reference cannot run the scene's mode (rich=False, below) or it died on this scene.  The reference runs in a server process of its
    own (tests/ref_worker.py): it aborts on some inputs it was never exercised on (degenerate random configurations), which must not
    end the test session."""
    import os
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    if not all(os.path.exists(os.path.join(os.path.dirname(here), "oracle", "_ref", b + ".so")) for b in R3D_BUILDS):
        return None
    if not rich:
        # the reference's 3D backward reads the per-triangle normal gradients unconditionally (R3D backward.cu:176) but allocates them
        # only with rich_info (rasterizer.cu:279-282): without it every backward reads unallocated device memory.  Its own Python module
        # never gets there (its backward needs the depth / normal gradients of rich_info).  These scenes are compared with the oracle.
        return None
    with tempfile.TemporaryDirectory() as tmp:
        scene, out = os.path.join(tmp, "scene.npz"), os.path.join(tmp, "ref.npz")
        np.savez(scene, __rich=rich, __back=back, __use_feature=use_feature, __variant=3,
                 **{k: np.asarray(v) for k, v in s.items() if v is not None})
        ans = _ref_request(f"{scene} {out} {','.join(R3D_BUILDS)}")
        if ans is None:
            return None  # killed by a signal: the caller falls back to the oracle
        assert ans == "ok" and os.path.exists(out), ans
        z = np.load(out)
        res = {b: {} for b in R3D_BUILDS}
        for key in z.files:
            b, k = key.split("/", 1)
            res[b][k] = int(z[key]) if k == "num_rendered" else z[key]
        return res


def _dist3d(k, x, y):
    """(distance, number of depth pixels set aside).  Depth only: a pixel whose ray lies nearly IN a triangle's plane (|p_ray.n| small but
    above the reference's absolute 1e-8 guard, R3D forward.cu:241-243) gets depth = v1.n / p_ray.n of 1e4 ... 1e11 in EVERY build, each with
    its own rounding noise, and one such pixel outweighs the rest of the map in an L2 norm: pixels that differ by more than 1e-3 of their (or
    the typical) depth are counted and the norm is taken over the others.  How many may be set aside is judged by the caller -- like the
    distances themselves, against what the reference's own builds do to each other."""
    if k == "depth":
        scale = np.maximum(np.abs(y), np.median(np.abs(y)))
        bad = ~(np.abs(x - y) <= 1e-3 * scale)
        return rel_l2(x[~bad], y[~bad]), int(bad.sum())
    return rel_l2(x, y), 0


def assert_inside_reference_spread_3d(hf, builds, what=""):
    """See the block comment above.  `hf`: the product's outputs, `builds`: ref3d_builds(...)."""
    names = list(builds)
    report = {}
    for k, tol in R3D_BARS.items():
        if k not in hf or any(k not in builds[b] for b in names):
            continue
        own_pairs = [_dist3d(k, builds[a][k], builds[b][k]) for i, a in enumerate(names) for b in names[i + 1:]]
        mine_pairs = [_dist3d(k, hf[k], builds[b][k]) for b in names]
        own, mine = [d for d, _ in own_pairs], [d for d, _ in mine_pairs]
        report[k] = (mine, own)
        assert min(mine) <= max(tol, float(np.median(own))), (what, k, "closest build", mine, own)
        assert max(mine) <= max(tol, 1.25 * max(own)), (what, k, "farthest build", mine, own)
        if k == "depth":
            # the pixels set aside: at most 1e-4 of the map (at least one) -- or as many as the reference's builds set aside among themselves
            # (extended fuzz sweep: seed 93, 5 of 33 150 pixels between two builds of the reference, 1 - 4 for the product; seed 161, 0 - 1 of
            # 7 905 between builds, 1 - 2 for the product -- counts this small scatter by a factor two between any two evaluations)
            size = int(np.asarray(hf[k]).size)
            budget = max(1, int(1e-4 * size))
            own_bad, mine_bad = [n for _, n in own_pairs], [n for _, n in mine_pairs]
            assert min(mine_bad) <= max(budget, int(np.median(own_bad))), (what, k, "pixels set aside, closest build", mine_bad, own_bad)
            assert max(mine_bad) <= max(budget, 2 * max(own_bad)), (what, k, "pixels set aside, farthest build", mine_bad, own_bad)
    return report
