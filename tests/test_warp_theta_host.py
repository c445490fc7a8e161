"""The float64 restatement of the affine warp's gradient in theta (tests/warp_theta_ref.py) against yardsticks that share
nothing with it, and the library's refusals; no GPU.

  torch fp64 autograd   grid_sample(align_corners=True, padding_mode="zeros") of x - fill on the grid of the voxel theta
  central differences   of affine_ref.affine_warp_ref in each of the 12 entries, on the rotated cases
  a right-hand difference on the integer-valued thetas, which pins the derivative's side at an integer coordinate"""
import ctypes
import os

import numpy as np
import pytest
import torch

import affine_ref as R
import warp_theta_ref as T


def _autograd(x, gy, theta, fill):
    """sum(gy * warp(x, theta)) differentiated in theta by torch, fp64: (n, 12)."""
    n, S, O = x.shape[0], x.shape[1:], gy.shape[1:]
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None] - fill
    th = torch.tensor(np.asarray(theta, dtype=np.float64).reshape(n, 3, 4), requires_grad=True)
    p = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in O], indexing="ij")
                    + (torch.ones(O, dtype=torch.float64),), dim=-1)                      # (oD, oH, oW, 4)
    c = torch.einsum("nkj,dhwj->ndhwk", th, p)                                            # (n, oD, oH, oW, 3) in (d, h, w)
    if S[0] == 1:                                                                         # 2-D: (h, w) only
        size = torch.tensor([S[2] - 1, S[1] - 1], dtype=torch.float64)
        grid = 2.0 * c[:, 0, :, :, [2, 1]] / size - 1.0                                   # grid_sample wants (x = w, y = h)
        y = torch.nn.functional.grid_sample(xt[:, :, 0], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        y = y[:, :, None]
    else:
        size = torch.tensor([S[2] - 1, S[1] - 1, S[0] - 1], dtype=torch.float64)
        grid = 2.0 * c[..., [2, 1, 0]] / size - 1.0
        y = torch.nn.functional.grid_sample(xt, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    (y[:, 0] * torch.from_numpy(np.asarray(gy, dtype=np.float64))).sum().backward()
    return th.grad.reshape(n, 12).numpy()


@pytest.mark.parametrize("fill", T.FILLS)
@pytest.mark.parametrize("name", ["rot3d", "crop", "zoom2", "mini", "rot2d"])
def test_restatement_against_torch_autograd(name, fill):
    """|ref - autograd| <= 1e-10 on every entry (measured: at most 1e-13 on entries up to 90).  rot2d: rows h and w only,
    the size-1 axis has no meaning in grid_sample's normalised coordinates."""
    n, in_size, out_size, theta = T.CASES[name]
    x, _, gy, _ = T.make_case(name)
    ref, scale = T.affine_warp_theta_grad_ref(x, gy, theta, fill)
    got = _autograd(x, gy, theta, fill)
    rows = slice(4, 12) if in_size[0] == 1 else slice(0, 12)
    err = np.abs(ref - got)[:, rows]
    print(f"{name} fill {fill}: max |ref - autograd| = {err.max():.3e}, max |ref| = {np.abs(ref[:, rows]).max():.3f}")
    assert np.abs(ref[:, rows]).max() > 1.0 and err.max() <= 1e-10


@pytest.mark.parametrize("fill", T.FILLS)
@pytest.mark.parametrize("name", ["rot3d", "rot2d", "crop", "zoom2", "mini", "tiles3d"])
def test_restatement_against_central_differences(name, fill):
    """Within a cell y is linear in one entry of theta (that entry moves one c_k alone), so a central difference with step
    1e-6 is exact but for the rounding of y (1e-16 / 1e-6 per term): agreement 1e-6 relative to the sum of |terms|."""
    n, in_size, out_size, theta = T.CASES[name]
    x, _, gy, _ = T.make_case(name)
    ref, scale = T.affine_warp_theta_grad_ref(x, gy, theta, fill)
    h = 1e-6
    worst = 0.0
    for e in range(12):
        if in_size[0] == 1 and e < 4:
            continue                                  # D = 1: moving c_d off 0 leaves the image's plane, a one-sided matter
        up, dn = theta.copy(), theta.copy()
        up[:, e] += h
        dn[:, e] -= h
        yu = R.affine_warp_ref(x, up, out_size, mode=R.CONSTANT, fill=fill)
        yd = R.affine_warp_ref(x, dn, out_size, mode=R.CONSTANT, fill=fill)
        fd = ((yu - yd) * gy).reshape(n, -1).sum(axis=1) / (2 * h)
        gap = np.abs(fd - ref[:, e])
        worst = max(worst, float((gap / np.maximum(scale[:, e], 1e-300)).max()))
        assert (gap <= 1e-6 * scale[:, e]).all(), (name, e, fd, ref[:, e], scale[:, e])       # (D = 1, j = 0: 0 <= 0)
    print(f"{name} fill {fill}: worst |fd - ref| / sum |terms| = {worst:.3e}")


@pytest.mark.parametrize("fill", T.FILLS)
def test_integer_thetas_take_the_right_hand_derivative(fill):
    """Every coordinate is an integer and every f is 0: the forward reads one corner per voxel, the derivative lives in the
    seven others.  P >= 0, so raising an entry of theta moves c to the right: (y(theta + h e) - y(theta)) / h is the
    derivative on the cell [b, b + 1], exactly (y is linear there)."""
    n, in_size, out_size, theta = T.CASES["integer"]
    x, _, gy, _ = T.make_case("integer")
    ref, scale = T.affine_warp_theta_grad_ref(x, gy, theta, fill)
    y0 = R.affine_warp_ref(x, theta, out_size, mode=R.CONSTANT, fill=fill)
    h = 1e-6
    for e in range(12):
        up = theta.copy()
        up[:, e] += h
        fd = ((R.affine_warp_ref(x, up, out_size, mode=R.CONSTANT, fill=fill) - y0) * gy).reshape(n, -1).sum(axis=1) / h
        assert (np.abs(fd - ref[:, e]) <= 1e-6 * scale[:, e] + 1e-12).all(), (e, fd, ref[:, e])
    assert (scale[:, [3, 7, 11]] > 1.0).all()          # the derivative is there although every forward weight beside 1 is 0
    # the left-hand difference is another number: the convention is a choice
    dn = theta.copy()
    dn[:, 11] -= h
    left = ((y0 - R.affine_warp_ref(x, dn, out_size, mode=R.CONSTANT, fill=fill)) * gy).reshape(n, -1).sum(axis=1) / h
    assert (np.abs(left - ref[:, 11]) > 1e-3).all()


def test_dead_voxels_and_the_two_plane_sum():
    n, in_size, out_size, theta = T.CASES["nan"]
    x0, x1, g0, g1 = T.make_case("nan")
    ref, scale = T.affine_warp_theta_grad_ref(x0, g0, theta, -1.0)
    assert not ref[0].any() and not scale[0].any() and np.abs(ref[1]).max() > 0.1
    both, _ = T.affine_warp_theta_grad_ref(x0, g0, theta, -1.0, x1, g1, 0.5)
    other, _ = T.affine_warp_theta_grad_ref(x1, g1, theta, 0.5)
    assert np.abs(both - (ref + other)).max() <= 1e-12
    # a 2-D image: the j = 0 column is 0 (d = 0), the k = 0 row is fill - x at the only d corner pair
    n, in_size, out_size, theta = T.CASES["rot2d"]
    x0, _, g0, _ = T.make_case("rot2d")
    ref, _ = T.affine_warp_theta_grad_ref(x0, g0, theta, -1.0)
    assert not ref[:, [0, 4, 8]].any() and np.abs(ref[:, 1:4]).max() > 0.1


# ---- the library's refusals (host side, before any launch) ---------------------------------------------------------------
def test_library_refusals():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmpgan_hip.so not built (run __graft_entry__.build())")
    lib = _lib.lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    assert lib.mpgan_affine_warp_theta_workspace(2, i3(7, 9, 11)) == 2 * 2 * 2 * 1 * 12 * 8      # 4 x 8 x 32 tiles
    assert lib.mpgan_affine_warp_theta_workspace(3, i3(1, 13, 10)) == 3 * 2 * 12 * 8              # 1 x 8 x 32 tiles
    assert lib.mpgan_affine_warp_theta_workspace(2, i3(1, 264, 250)) == 2 * 264 * 12 * 8
    assert lib.mpgan_affine_warp_theta_workspace(0, i3(7, 9, 11)) == -1
    assert lib.mpgan_affine_warp_theta_workspace(1, i3(7, 0, 11)) == -1
    assert lib.mpgan_affine_warp_theta_workspace(1, None) == -1
    assert lib.mpgan_affine_warp_theta_workspace(2, i3(1024, 1024, 1024)) == -1
    p = ctypes.c_void_p(4096)                         # never dereferenced: every call below is refused on the host
    need = 2 * 4 * 12 * 8

    def call(**kw):
        a = dict(x0=p, x1=None, gy0=p, gy1=None, n=2, in_dhw=i3(7, 9, 11), out_dhw=i3(7, 9, 11), theta=p, mode=0, ws=p,
                 ws_bytes=need, gtheta=p)
        a.update(kw)
        return lib.mpgan_affine_warp_backward_theta(a["x0"], a["x1"], a["gy0"], a["gy1"], a["n"], a["in_dhw"], a["out_dhw"],
                                                    a["theta"], a["mode"], -1.0, -1.0, a["ws"], a["ws_bytes"], a["gtheta"],
                                                    None)

    cases = [(dict(x0=None), b"null"), (dict(gy0=None), b"null"), (dict(theta=None), b"null"), (dict(gtheta=None), b"null"),
             (dict(in_dhw=None), b"null"), (dict(out_dhw=None), b"null"), (dict(x1=p), b"go together"),
             (dict(gy1=p), b"go together"), (dict(n=0), b"n = 0"), (dict(in_dhw=i3(7, 0, 11)), b"extent"),
             (dict(out_dhw=i3(0, 9, 11)), b"extent"), (dict(mode=2), b"unknown mode"), (dict(mode=1), b"border"),
             (dict(ws=None), b"workspace"), (dict(ws_bytes=need - 8), b"workspace"),
             (dict(ws=ctypes.c_void_p(4100)), b"aligned"), (dict(in_dhw=i3(1024, 1024, 1024)), b"32-bit"),
             (dict(out_dhw=i3(1024, 1024, 1024)), b"32-bit")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = lib.mpgan_last_error()
        assert b"mpgan_affine_warp_backward_theta" in msg and word in msg, (kw, msg)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpgan_hip.h")).read()
    assert "mpgan_affine_warp_backward_theta" in header and "mpgan_affine_warp_theta_workspace" in header
