"""The blend backward with the eight per-pixel "behind" recurrences folded into one (surfel_math.h BwdPixel::u, bwd_dot):
dL/dalpha's eight terms (f - x) g are phi - u, with phi the entry's features dotted with the pixel's upstream gradients and
u the same dot of what lies behind, carried by the same recurrence u <- u + alpha (phi - u).
  * host: the product's header walked with the new and with the eight-value formulation over the same pairs -- the 20
    accumulator components agree to 2e-6 of each component's scale, in every instance (FULL, GEOM, LITE);
  * GPU: the backward against the CPU oracle at the usual tolerances, on saturating scenes, on long lists whose recorded
    segments start mid-list (u initialised from the segments' suffix sums), in every instance, with the paired forward
    feeding the recorded backward."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import surfel_oracle as so
from tests.host_emul import emul
from tests.util import assert_close, make_case, oracle_forward
from vidu4d_amd.synthetic import make_scene, make_upstream_grads

_HERE = os.path.dirname(os.path.abspath(__file__))
_MODES = {"full": 0, "lite": 1, "geom": 2}            # surfel_math.h BLEND_FULL, BLEND_LITE, BLEND_GEOM
_KEEP = {"full": list(range(8)), "lite": [1], "geom": [0, 1, 2, 3, 4]}   # upstream planes each instance reads
_lib = None


def _host_lib():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "host_emul", "bwd_projected.cpp")
        out = os.path.join(tempfile.mkdtemp(prefix="bwd_projected_"), "libbwd_projected.so")
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-mfma",
                               "-Wno-unknown-pragmas", "-o", out, src])
        _lib = C.CDLL(out)
    return _lib


def _zero_dead_planes(do, mode):
    z = torch.zeros_like(do)
    z[_KEEP[mode]] = do[_KEEP[mode]]
    return z


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("mode", ["full", "geom", "lite"])
@pytest.mark.parametrize("case", ["ragged", "deg2", "huge", "init_opacity", "opaque"])
def test_projected_recurrence_equals_the_eight_running_values_on_the_host(case, mode):
    if case == "opaque":
        sc = make_scene(1500, 96, 64, seed=7, sigma_px=4.0)
        sc.opacities[:] = 0.98      # near-1 opacities: every covered pixel saturates after a few entries
    else:
        sc = make_case(case)
    st = oracle_forward(sc)
    dc, do = make_upstream_grads(sc.width, sc.height)
    do = _zero_dead_planes(do, mode)
    e = emul.run(st, dc.numpy(), do.numpy(), lite=mode == "lite")   # (the emulated forward state: final_T, n_contrib, rec)
    P, W, H = st["P"], st["W"], st["H"]
    new, eight = np.zeros((P, 20)), np.zeros((P, 20))
    _host_lib().bwd_projected_walk(
        C.c_int(_MODES[mode]), C.c_int(W), C.c_int(H), _p(st["ranges"]), _p(st["point_list"]), _p(e["rec"]),
        _p(np.ascontiguousarray(st["_inputs"]["bg"], np.float32)), _p(e["final_T"]), _p(e["n_contrib"]),
        _p(np.ascontiguousarray(dc.numpy(), np.float32)), _p(np.ascontiguousarray(do.numpy(), np.float32)), _p(new), _p(eight))
    assert np.abs(eight).max() > 0
    # (the walk is the one emul.run's backward took: same accumulators, cull aside -- which drops nothing)
    assert np.allclose(new.astype(np.float32), e["acc"], rtol=0, atol=1e-6 * float(np.abs(e["acc"]).max()))
    scale = np.abs(eight).max(axis=0) + 1e-30
    err = np.abs(new - eight) / scale
    assert (err <= 2e-6).all(), err.max(axis=0)


# ------------------------------------------------------------------------------------------------------------ GPU

def _gpu_scene(which):
    if which == "opaque_slab":
        sc = make_scene(60_000, 256, 192, seed=41, sigma_px=6.0)
        sc.opacities[:] = 0.98                       # near-1 opacities: pixels saturate a few entries into long lists
        return sc
    if which == "saturating":
        sc = make_scene(40_000, 192, 128, seed=32, sigma_px=5.0)
        sc.opacities[:] = 0.9
        return sc
    if which == "long_lists":
        return make_scene(60_000, 256, 256, seed=31)   # lists of ~700 entries: several recorded segments per tile
    sc = make_scene(30_000, 160, 128, seed=91, sigma_px=1.0)   # everything into a few tiles: lists of thousands
    g = torch.Generator().manual_seed(91)
    sc.means3D[:, 0] = (torch.rand(30_000, generator=g) - 0.5) * 0.25 * sc.means3D[:, 2]
    sc.means3D[:, 1] = (torch.rand(30_000, generator=g) - 0.5) * 0.25 * sc.means3D[:, 2]
    sc.opacities[:] = 0.1
    return sc


def _native(sc, dev, aux, dc, do):
    from vidu4d_amd import _C
    d = sc.to(dev)
    e = torch.empty(0, device=dev)
    out = _C.rasterize_gaussians(d.bg, d.means3D, e, d.opacities, d.scales, d.rotations, 1.0, e, d.viewmatrix, d.projmatrix,
                                 sc.tanfovx, sc.tanfovy, sc.height, sc.width, d.shs, sc.sh_degree, d.campos, False, False,
                                 aux_planes=aux)
    R, color, others, radii, geom, binning, img = out
    g = _C.rasterize_gaussians_backward(d.bg, d.means3D, radii, e, d.scales, d.rotations, 1.0, e, d.viewmatrix,
                                        d.projmatrix, sc.tanfovx, sc.tanfovy, dc.to(dev), do.to(dev), d.shs, sc.sh_degree,
                                        d.campos, geom, R, binning, img, False, aux_planes=aux)
    header = geom[:256].view(torch.int32).cpu()
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dtransMat", "dL_dsh", "dL_dscales",
             "dL_drotations"]
    return dict(zip(names, g)), header


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("mode", ["full", "geom", "lite"])
@pytest.mark.parametrize("which", ["opaque_slab", "saturating", "long_lists", "concentrated"])
def test_projected_backward_matches_the_oracle(gpu_device, monkeypatch, which, mode, paired):
    """Whole-tile forward (which leaves recorded segments on long lists) feeding the recorded backward, and the same with
    every tile's forward paired (two workgroups per tile): gradients against the oracle's backward with the instance's dead
    upstream planes zeroed."""
    from vidu4d_amd import _C, _lib
    monkeypatch.setattr(_C, "_SPLIT", "0")
    monkeypatch.setattr(_C, "PAIR_K", 15 if paired else 0)
    aux = {"full": 0, "lite": _lib.AUX_ALPHA, "geom": _lib.AUX_GEOM}[mode]
    sc = _gpu_scene(which)
    st = oracle_forward(sc)
    dc, do = make_upstream_grads(sc.width, sc.height)
    do = _zero_dead_planes(do, mode)
    want = so.backward(st, dc, do)
    got, header = _native(sc, gpu_device, aux, dc, do)
    if which in ("long_lists", "concentrated"):
        assert int(header[5]) == 2, "the scene must leave recorded segments (Header::split_used)"
    if paired:
        assert int(header[17]) > 0, "the forward must have paired tiles (Header::num_paired)"
    for k, t in got.items():
        if mode != "full" and k == "dL_dtransMat":
            continue   # (not compared for these instances, as in tests/test_host_math.py)
        assert torch.isfinite(t).all(), k
        assert_close(k, t, want[k])
