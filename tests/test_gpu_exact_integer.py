"""Exact-arithmetic tests of the field kernels: every element, bit for bit.

The other suites gate the training kernels with norms (relative L2 of 2e-2 for bf16), which cannot see a few wrong
elements of a gradient tensor.  Here the inputs are chosen so that every kernel's arithmetic is EXACT: weights, biases,
coordinates, upstream gradients and every intermediate value are integers of magnitude at most 256.  Such values are
exact bf16 MFMA operands (8 significant bits), exact fp16 operands (the split pairs have lo = 0) and exact fp32
operands; every product and partial sum is an integer below 2^24, so fp32 accumulation is exact in any order -- slab
reductions, atomically accumulated ray gradients and the power-of-two loss scale of the split backward included.  A
correct kernel then reproduces the float64 reference element by element in all three precisions: the tolerance is
zero, and zero is derived, not measured.

What the exact claim does not cover: the sin / cos columns of the three tensors that read a positional encoding
(pts_linears.0, the layer after the skip, views_linears.0).  The network's weights on those columns are zero, which
removes the (non-integer) encoded values from the forward, the dX chain and the point gradients exactly -- but the
weight GRADIENT there is an integer gradient times a non-integer encoding.  Those columns stay under the relative-L2
gate the existing tests apply to that precision and tensor (SINCOS_GATE); nothing here says anything about rounding
on non-integer data, where the rounding-model and fp64 tests remain the authority.

CPU tests (no marker) check the generator: the preconditions under which exactness is owed, the caps that keep the
test from being vacuous, and that the comparison helper names the first differing index.
"""
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

from oracle import nerf_oracle as O  # noqa: E402
from test_gpu_fuzz import SIZES as FUZZ_SIZES  # noqa: E402
from test_gpu_train_f32 import ARCHS as F32_ARCHS  # noqa: E402

gpu = pytest.mark.gpu

_VD = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)
_NOVD = dict(_VD, use_viewdirs=False)
# the fused 8 x 256 family: trains in bf16, fp32_split and fp32
FUSED = {
    "vd_10_4": _VD,
    "vd_15_6": dict(_VD, multires=15, multires_views=6),
    "novd_out5": _NOVD,
    "novd_out4": dict(_NOVD, output_ch=4),
    "novd_15_out13": dict(_NOVD, multires=15, output_ch=13),       # the third tile row group of output_linear
}
# architectures of csrc/train_f32.hip (exact-fp32 training path); the identity embedding makes every column exact
F32 = {k: F32_ARCHS[k] for k in ("d4_w128_skip2", "d6_w96_skips13", "d3_w320_skip0", "d2_w600_wide", "d2_w1024_widest",
                                 "d8_w256_identity_embed")}
ARCHS = {**FUSED, **F32}
PRECISIONS = {name: (("bf16", "fp32_split", "fp32") if name in FUSED else ("fp32",)) for name in ARCHS}
WEIGHT_SEED = {name: 100 + i for i, name in enumerate(ARCHS)}

# (rays, samples) of every training case: the awkward counts of tests/test_gpu_fuzz.py (one point, the 32-point chunks
# of the weight-gradient products, the 256-point tiles, ragged tails), plus one count just past each boundary at which
# a launcher changes shape:
#   481   csrc/dw_plan.h DwPlan::layout (both precisions): a job gets at most n_chunks / 8 workgroups, so the 16th
#         32-point chunk (point 481) brings the second workgroup and the second slab to reduce; from there on every
#         workgroup streams more chunks than one (the strided chunk loop of dw2_body / dw2s_body)
#   1025  csrc/train_f32.hip dw_slice_pts: 1024 points per weight-gradient slice, so the second slice (blockIdx.y = 1)
#   5633  dw_plan.h dw_share_workgroups (tools/dw_plan_check.cpp prints the shares).  View-branch model, 13 jobs, cap
#         n_chunks / 8 = 22: the 256 workgroups run out, the wide jobs sit at the cap and the cost table deals the rest
#         (bf16: 19 22 22 22 22 18 22 22 22 22 22 12 9).  The output_linear model's 9 jobs all sit at the cap: 198
#   7500  cap 29: the output_linear model's workgroups run out too (27 29 29 29 29 26 29 29 29), and the view-branch
#         model has the shares of a full-size step, which the cap no longer touches (15 24 24 24 24 14 24 24 24 26 17 9 7)
#   (257 -- second row of dw_small_kernel's 256-point grid, second tile of the dX chain -- is in the fuzz list; the
#   1024-workgroup cap of launch_dw_small and the 32768-slice cap of dw_slice_pts lie beyond 2.6e5 points, where the
#   2^24 precondition no longer holds)
SIZES = list(FUZZ_SIZES) + [(13, 37), (25, 41), (43, 131), (60, 125)]
assert max(r * s for r, s in SIZES) < 10000

# Whole-tensor relative L2 of the three encoding-reading weight gradients, whose sin / cos columns are not exact: the
# gates of test_gpu_backward.py::test_field_backward_matches_autograd (bf16, against the bf16 rounding model),
# test_gpu_split_backward.py GATE_REL (fp32_split) and test_gpu_train_f32.py::check (fp32).  Every other column of
# these tensors has been compared exactly before, so all of the error the gate sees sits in the sin / cos columns.
SINCOS_GATE = {"bf16": 2e-2, "fp32_split": 1e-3, "fp32": 2e-5}


# ------------------------------------------------------------------------------------------------ the integer network
def _arch(arch):
    return O.Arch(**{**arch, "skips": tuple(arch["skips"])})


def layer_table(arch, dense_inputs=False):
    """[(name, n_out, n_in, live input columns, first encoding column or None, encoding width, kind)] in forward order.
    Live columns of a layer that reads a positional encoding: the three identity columns of that encoding plus all
    hidden columns (dense_inputs: every column -- NeRF.MLP's caller supplies the 'encoding' itself)."""
    A = _arch(arch)
    W, ic, icv = A.W, A.input_ch, A.input_ch_views
    enc = lambda n: list(range(n if dense_inputs else min(n, 3)))       # noqa: E731
    rows = [("pts_linears.0", W, ic, enc(ic), 0, ic, "first")]
    for i in range(1, A.D):
        if (i - 1) in A.skips:
            rows.append(("pts_linears.%d" % i, W, W + ic, enc(ic) + list(range(ic, ic + W)), 0, ic, "hidden"))
        else:
            rows.append(("pts_linears.%d" % i, W, W, list(range(W)), None, 0, "hidden"))
    # (the reference builds views_linears.0 for every model, nerf.py:83; without view branch nothing reads it)
    rows.append(("views_linears.0", W // 2, W + icv, list(range(W)) + [W + c for c in enc(icv)], W if icv else None, icv, "hidden"))
    if A.use_viewdirs:
        rows += [("feature_linear", W, W, list(range(W)), None, 0, "hidden"), ("alpha_linear", 1, W, None, None, 0, "head"),
                 ("rgb_linear", 3, W // 2, None, None, 0, "head")]
    else:
        rows.append(("output_linear", A.output_ch, W, None, None, 0, "head"))
    return rows


def sincos_columns(arch):
    """{weight name: bool mask over input columns} for the tensors that read a sin / cos encoding."""
    A = _arch(arch)
    out = {}
    if A.i_embed == -1:
        return out
    for name, n_out, n_in, live, enc0, enc_w, kind in layer_table(arch):
        if enc0 is None or (name == "views_linears.0" and not A.use_viewdirs):
            continue
        mask = torch.zeros(n_in, dtype=torch.bool)
        mask[enc0 + 3:enc0 + enc_w] = True
        out[name + ".weight"] = mask
    return out


def integer_state_dict(arch, seed, dense_inputs=False):
    """Hand-built weights on which the network's arithmetic is exact.  Hidden layers: row o has +1 at column perm[o]
    (a random permutation of the live columns, repeated when there are fewer of them than rows) and one extra entry at a
    random live column, -1 with probability 0.6 and +1 otherwise (skipped when it lands on perm[o]); bias from
    {-1, 0, 0, 1}, for layer 0 from {0, 1, 2}.  Heads: dense rows from {-1, 0, 1} with probabilities .25 / .5 / .25.
    Weights on sin / cos columns are zero."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, n_out, n_in, live, _, _, kind in layer_table(arch, dense_inputs):
        if kind == "head":
            w = rng.choice([-1.0, 0.0, 1.0], p=[0.25, 0.5, 0.25], size=(n_out, n_in))
            b = rng.choice([-1.0, 0.0, 0.0, 1.0], size=n_out)
        else:
            live = np.asarray(live)
            reps = -(-n_out // len(live))
            perm = np.concatenate([rng.permutation(live) for _ in range(reps)])[:n_out]
            w = np.zeros((n_out, n_in))
            w[np.arange(n_out), perm] = 1.0
            extra = rng.choice(live, size=n_out)
            sign = np.where(rng.random(n_out) < 0.6, -1.0, 1.0)
            rows = np.nonzero(extra != perm)[0]
            w[rows, extra[rows]] = sign[rows]
            b = rng.choice([0.0, 1.0, 2.0] if kind == "first" else [-1.0, 0.0, 0.0, 1.0], size=n_out)
        sd[name + ".weight"] = torch.from_numpy(w.astype(np.float32))
        sd[name + ".bias"] = torch.from_numpy(b.astype(np.float32))
    return sd


def integer_inputs(arch, R, S, seed):
    """Points in [-3, 3], view directions in [-2, 2] (NeRF.forward does not normalise them), dL/draw in [-2, 2]."""
    rng = np.random.default_rng(seed)
    A = _arch(arch)
    pts = torch.from_numpy(rng.integers(-3, 4, size=(R, S, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.integers(-2, 3, size=(R, 3)).astype(np.float32)) if A.use_viewdirs else None
    g_raw = torch.from_numpy(rng.integers(-2, 3, size=(R, S, 4 if A.use_viewdirs else A.output_ch)).astype(np.float32))
    return pts, vd, g_raw


def integer_rays(arch, R, S, seed):
    """rays [R, 11] (view branch) or [R, 8], z_vals [R, S], dL/draw.  o in [-1, 1]; each ray draws a scale k in
    {1, 2, 4}, d = k * {-1, 0, 1}^3 and depths that are multiples of 1 / k in [0, 3 / k]: z_vals are multiples of 0.25
    in [0, 4] and d z is an integer in [-3, 3].  o + d z must be an integer, not just exact in fp32: bf16 keeps 8
    significant bits, so a hidden activation like 84.25 -- what a fractional coordinate leads to -- would not be an
    exact MFMA operand.  The depths themselves are fractional: dL/dd = sum_s z g_pts has quarters."""
    rng = np.random.default_rng(seed)
    A = _arch(arch)
    k = rng.choice([1.0, 2.0, 4.0], size=(R, 1))
    o = rng.integers(-1, 2, size=(R, 3)).astype(np.float64)
    d = k * rng.integers(-1, 2, size=(R, 3))
    z = np.sort(rng.integers(0, 4, size=(R, S)), -1) / k
    cols = [o, d, np.zeros((R, 1)), np.full((R, 1), 4.0)]
    if A.use_viewdirs:
        cols.append(rng.integers(-2, 3, size=(R, 3)).astype(np.float64))
    rays = torch.from_numpy(np.concatenate(cols, -1).astype(np.float32))
    g_raw = torch.from_numpy(rng.integers(-2, 3, size=(R, S, 4 if A.use_viewdirs else A.output_ch)).astype(np.float32))
    return rays, torch.from_numpy(z.astype(np.float32)), g_raw


# ------------------------------------------------------------------------------------------------ float64 reference
def net64(sd, arch, e_pts, e_dirs, tape=None, act=torch.relu):
    """NeRF.MLP (the reference's nerf.py:110-134) in float64 on encoded rows; `tape` collects (weight name, input,
    pre-activation, has ReLU) of every layer.  `act` stands in for the ReLU (partial_case: a recorded mask)."""
    A = _arch(arch)

    def lin(name, x, relu):
        z = torch.nn.functional.linear(x, sd[name + ".weight"], sd[name + ".bias"])
        if tape is not None:
            if z.requires_grad:
                z.retain_grad()
            tape.append((name, x, z, relu))
        return act(z) if relu else z

    h = e_pts
    for i in range(A.D):
        h = lin("pts_linears.%d" % i, h, True)
        if i in A.skips:
            h = torch.cat([e_pts, h], -1)
    if not A.use_viewdirs:
        return lin("output_linear", h, False)
    sigma = lin("alpha_linear", h, False)
    feat = lin("feature_linear", h, False)
    hv = lin("views_linears.0", torch.cat([feat, e_dirs], -1), True)
    return torch.cat([lin("rgb_linear", hv, False), sigma], -1)


def reference(arch, sd, pts, vd, g_raw):
    """Forward and backward in float64 with autograd: raw, every parameter gradient, g_pts, g_viewdirs, and the
    statistics the preconditions are stated on."""
    A = _arch(arch)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    p64 = pts.double().requires_grad_(True)
    v64 = vd.double().requires_grad_(True) if vd is not None else None
    flat = p64.reshape(-1, 3)
    e_pts = O.embed(flat, A.multires, A.i_embed)
    e_dirs = None
    if v64 is not None:
        e_dirs = O.embed(v64[:, None].expand(p64.shape).reshape(-1, 3), A.multires_views, A.i_embed)
    tape = []
    raw = net64(sd64, arch, e_pts, e_dirs, tape).reshape(list(pts.shape[:-1]) + [-1])
    (raw * g_raw.double()).sum().backward()
    sincos = sincos_columns(arch)
    st = dict(max_act=0.0, max_dx=0.0, max_prod=0.0, max_gw=0.0, live={}, share={})
    bf16_model = {}
    for name, x, z, relu in tape:
        head = name in ("alpha_linear", "rgb_linear", "output_linear")
        zg, z = z.grad, z.detach()
        if not head:
            st["max_act"] = max(st["max_act"], float((torch.relu(z) if relu else z).abs().max()))
        st["max_dx"] = max(st["max_dx"], float(zg.abs().max()))
        st["max_prod"] = max(st["max_prod"], float((zg.abs().T @ x.detach().abs()).max()))
        if relu:
            st["live"][name] = float((z > 0).double().mean())
        gw = sd64[name + ".weight"].grad
        exact = gw[:, ~sincos[name + ".weight"]] if name + ".weight" in sincos else gw
        st["max_gw"] = max(st["max_gw"], float(exact.abs().max()))
        st["share"][name] = float((exact != 0).double().mean())
        if name + ".weight" in sincos:
            # the rounding model the bf16 gate is stated against: the encoding as the kernel holds it, rounded to bf16
            x32 = x.detach().float().to(torch.bfloat16).double()
            bf16_model[name + ".weight"] = zg.T @ x32
    grads = {k: v.grad.detach() for k, v in sd64.items() if v.grad is not None}
    return dict(raw=raw.detach(), grads=grads, g_pts=p64.grad.detach(), g_vd=v64.grad.detach() if v64 is not None else None,
                stats=st, sincos=sincos, bf16_model=bf16_model)


_CACHE = {}
INFER_SIZES = [(1, 1), (17, 241), (100, 97)]          # the training cases the inference tests read too


def case(name, R, S):
    """(state dict, pts, viewdirs, dL/draw, reference) of one training case; computed once and shared, never modified."""
    key = (name, R, S)
    if key not in _CACHE:
        arch = ARCHS[name]
        sd = weights(name)
        pts, vd, g_raw = integer_inputs(arch, R, S, 1000 * WEIGHT_SEED[name] + 97 * R + S)
        _CACHE[key] = (sd, pts, vd, g_raw, reference(arch, sd, pts, vd, g_raw))
    return _CACHE[key]


def forget(name, R, S):
    """Drop a training case that no other test reads (a reference holds every gradient of the model in float64)."""
    if (R, S) not in INFER_SIZES:
        _CACHE.pop((name, R, S), None)


def weights(name):
    key = ("weights", name)
    if key not in _CACHE:
        _CACHE[key] = integer_state_dict(ARCHS[name], WEIGHT_SEED[name])
    return _CACHE[key]


def is_integer(t):
    return bool((t == t.round()).all())


def check_exactness_owed(arch, ref):
    """The conditions under which a correct kernel owes the float64 result bit for bit."""
    st = ref["stats"]
    assert st["max_act"] <= 256, st["max_act"]                  # exact bf16 / fp16 operands, forward
    assert st["max_dx"] <= 256, st["max_dx"]                    # ... and in the dX chain
    assert st["max_prod"] < 2 ** 24, st["max_prod"]             # |G|^T |X|: every partial sum of a weight gradient
    assert is_integer(ref["raw"]) and float(ref["raw"].abs().max()) < 2 ** 24
    assert is_integer(ref["g_pts"]) and (ref["g_vd"] is None or is_integer(ref["g_vd"]))
    for k, g in ref["grads"].items():
        exact = g[:, ~ref["sincos"][k]] if k in ref["sincos"] else g
        assert is_integer(exact), k


def check_not_vacuous(ref):
    """Caps (not measurements) that keep a draw from being trivially exact: hidden layers neither dead nor linear,
    weight gradients mostly nonzero."""
    st = ref["stats"]
    assert st["max_gw"] < 2 ** 24
    for name, frac in st["live"].items():
        assert 0.25 <= frac <= 0.75, (name, frac)
    for name, share in st["share"].items():
        assert share >= 0.4, (name, share)


# ------------------------------------------------------------------------------------------------ the comparison
def assert_exact(name, got, ref):
    """Numerical equality of every element after .double() (so -0 equals 0); on failure the tensor's name, the first
    differing index and (got, reference, difference) there -- the index is the diagnosis."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, "%s: shape %s, reference %s" % (name, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)                       # (a NaN differs from everything)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    g, r = float(got[idx]), float(ref[idx])
    raise AssertionError("%s differs at %d of %d elements; first at index %s: got %r, reference %r, difference %r"
                         % (name, int(bad.sum()), bad.numel(), idx, g, r, g - r))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def assert_param_grads(tag, named_grads, ref, precision, scale=1.0):
    """Every bias gradient and every weight-gradient element outside the sin / cos columns: exact.  The sin / cos
    columns (integer gradients times non-integer encodings: exactness is not owed) stay under the gate the existing
    tests apply to that precision and tensor."""
    for k, g in named_grads:
        if k not in ref["grads"]:
            assert g is None, "%s %s: a gradient for a parameter the reference does not reach" % (tag, k)
            continue
        assert g is not None, "%s %s: no gradient" % (tag, k)
        want = ref["grads"][k] * scale
        if k in ref["sincos"]:
            mask = ref["sincos"][k]
            assert_exact("%s %s [exact columns]" % (tag, k), g.detach().cpu()[:, ~mask], want[:, ~mask])
            model = ref["bf16_model"][k] * scale if precision == "bf16" else want
            e = rel_l2(g, model)
            print("%s %s sin/cos columns: relative L2 %.3e (gate %.0e)" % (tag, k, e, SINCOS_GATE[precision]))
            assert e < SINCOS_GATE[precision], (tag, k, e)
        else:
            assert_exact("%s %s" % (tag, k), g, want)


# ================================================================================================ CPU: the generator
CASES = [(name, R, S) for name in ARCHS for R, S in SIZES]
CASE_IDS = ["%s-%dx%d" % c for c in CASES]
# the caps of check_not_vacuous are statements about populations: they are asserted where a layer has one (the counts
# the recipe was designed at, 910 points and up); a single point cannot have half its units alive in every layer
NOT_VACUOUS_FROM = 900


@pytest.mark.parametrize("name,R,S", CASES, ids=CASE_IDS)
def test_generator_meets_the_preconditions(name, R, S):
    """Every architecture, seed and point count the GPU tests use: exactness is owed (integers, magnitudes at most 256,
    partial sums below 2^24), and from 900 points on the draw is not vacuous."""
    sd, pts, vd, g_raw, ref = case(name, R, S)
    for k, m in sincos_columns(ARCHS[name]).items():
        assert float(sd[k][:, m].abs().max()) == 0.0, k
    assert all(is_integer(v) for v in sd.values())
    check_exactness_owed(ARCHS[name], ref)
    if R * S >= NOT_VACUOUS_FROM:
        check_not_vacuous(ref)
    forget(name, R, S)


def rays_case(name, R, S):
    key = ("rays", name, R, S)
    if key not in _CACHE:
        arch = ARCHS[name]
        rays, z, g_raw = integer_rays(arch, R, S, 77 + 31 * R + S)
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
        vd = rays[:, 8:11].contiguous() if arch["use_viewdirs"] else None
        ref = reference(arch, weights(name), pts, vd, g_raw)
        g6 = torch.cat([ref["g_pts"].sum(1), (ref["g_pts"] * z.double()[..., None]).sum(1)], -1)
        g_rays = torch.cat([g6, torch.zeros(R, 2, dtype=torch.float64)] + ([ref["g_vd"]] if vd is not None else []), -1)
        _CACHE[key] = (rays, z, g_raw, pts, vd, ref, g_rays)
    return _CACHE[key]


# one tile of 256 points spans several rays (7 samples per ray); one ray spans several tiles (300 samples; 30 such rays,
# because a ray passes through at most seven integer points and the caps of check_not_vacuous need a population)
RAYS_CASES = [("vd_10_4", 300, 7), ("vd_10_4", 30, 300), ("novd_out5", 300, 7), ("novd_out5", 30, 300), ("vd_15_6", 41, 23)]


@pytest.mark.parametrize("name,R,S", RAYS_CASES)
def test_rays_generator_meets_the_preconditions(name, R, S):
    rays, z, g_raw, pts, vd, ref, g_rays = rays_case(name, R, S)
    assert is_integer(pts) and is_integer(z * 4) and float(z.min()) >= 0 and float(z.max()) <= 4
    assert not is_integer(z), "the depths are meant to be fractional"
    check_exactness_owed(ARCHS[name], ref)
    check_not_vacuous(ref)
    assert is_integer(g_rays * 4) and float(g_rays.abs().max()) < 2 ** 22       # quarters below 2^24 / 4: exact in fp32


def embedded_case(name, P):
    """Already-embedded integer rows for NeRF.MLP: the caller supplies the 'encoding', so every input column is live."""
    key = ("embedded", name, P)
    if key not in _CACHE:
        arch = ARCHS[name]
        A = _arch(arch)
        sd = integer_state_dict(arch, 500 + WEIGHT_SEED[name], dense_inputs=True)
        x = torch.from_numpy(np.random.default_rng(9).integers(-3, 4, size=(P, A.input_ch + A.input_ch_views)).astype(np.float32))
        tape = []
        with torch.no_grad():
            raw = net64({k: v.double() for k, v in sd.items()}, arch, x[:, :A.input_ch].double(), x[:, A.input_ch:].double(), tape)
        acts = [float((torch.relu(z) if relu else z).abs().max()) for _, _, z, relu in tape]
        used = {n: float((sd[n + ".weight"] != 0).any(0).double().mean()) for n in ("pts_linears.0", "views_linears.0")}
        _CACHE[key] = (sd, x, raw, max(acts), used)
    return _CACHE[key]


EMBEDDED = [("vd_10_4", 777), ("novd_out5", 300), ("d4_w128_skip2", 333)]


@pytest.mark.parametrize("name,P", EMBEDDED)
def test_embedded_generator_meets_the_preconditions(name, P):
    sd, x, raw, max_act, used = embedded_case(name, P)
    assert is_integer(raw) and max_act < 2 ** 24 and float(raw.abs().max()) < 2 ** 24      # the exact-fp32 kernel: fp32 range
    assert used["pts_linears.0"] == 1.0, used       # every encoding column carries a weight


INFER_EXTRA = {"novd_out20": dict(_NOVD, output_ch=20)}       # output_ch above 16: the 32x32x16 stream, inference only
ARCHS.update(INFER_EXTRA)
WEIGHT_SEED["novd_out20"] = 150
PRECISIONS["novd_out20"] = ("bf16", "fp32_split", "fp32")


@pytest.mark.parametrize("name", sorted(INFER_EXTRA))
@pytest.mark.parametrize("R,S", INFER_SIZES)
def test_inference_only_generator_meets_the_preconditions(name, R, S):
    sd, pts, vd, g_raw, ref = case(name, R, S)
    check_exactness_owed(ARCHS[name], ref)
    if R * S >= NOT_VACUOUS_FROM:
        check_not_vacuous(ref)


def test_the_comparison_names_the_first_wrong_element():
    """Sensitivity, shown on the comparison and not on a kernel: one added to a single element of a reference weight
    gradient, of a bias gradient and of the last point's raw fails the comparison and prints that index."""
    sd, pts, vd, g_raw, ref = case("vd_10_4", 70, 13)
    named = [(k, g.float()) for k, g in ref["grads"].items()]       # what a correct kernel returns: the integers, in fp32
    assert_param_grads("self", named, ref, "fp32")
    assert_exact("raw", ref["raw"].float(), ref["raw"])

    def perturbed(key, idx):
        r = dict(ref, grads={k: v.clone() for k, v in ref["grads"].items()})
        r["grads"][key][idx] += 1.0
        return r

    with pytest.raises(AssertionError, match=r"pts_linears\.3\.weight differs at 1 of 65536 elements; first at index \(201, 17\): "
                                             r"got .*, reference .*, difference -1\.0"):
        assert_param_grads("self", named, perturbed("pts_linears.3.weight", (201, 17)), "fp32")
    # an exact column of an encoding-reading tensor: column 258 of views_linears.0 is the third identity column of the directions
    with pytest.raises(AssertionError, match=r"views_linears\.0\.weight \[exact columns\] differs at 1 of .* index \(127, 258\)"):
        assert_param_grads("self", named, perturbed("views_linears.0.weight", (127, 258)), "fp32")
    with pytest.raises(AssertionError, match=r"feature_linear\.bias differs at 1 of 256 elements; first at index \(255,\)"):
        assert_param_grads("self", named, perturbed("feature_linear.bias", (255,)), "fp32")
    raw = ref["raw"].clone()
    raw[69, 12, 3] += 1.0
    with pytest.raises(AssertionError, match=r"raw differs at 1 of 3640 elements; first at index \(69, 12, 3\)"):
        assert_exact("raw", ref["raw"].float(), raw)
    with pytest.raises(AssertionError, match="raw differs"):       # a NaN is a difference, -0 is not
        assert_exact("raw", torch.full((2,), float("nan")), torch.zeros(2))
    assert_exact("raw", -torch.zeros(2), torch.zeros(2))


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_MODELS = {}


def gpu_model(dev, name, sd=None, tag=""):
    """The package's NeRF holding the integer weights (one per architecture, shared: the tests only change its precision)."""
    from nerf_shared_amd import nerf
    if (name, tag) not in _MODELS:
        m = nerf.NeRF(**ARCHS[name])
        m.load_state_dict(sd if sd is not None else weights(name))
        _MODELS[(name, tag)] = m.to(dev)
    m = _MODELS[(name, tag)]
    m.zero_grad(set_to_none=True)
    return m


def named_grads(m):
    return [(k, p.grad) for k, p in m.named_parameters()]


@gpu
@pytest.mark.parametrize("name,R,S", CASES, ids=CASE_IDS)
def test_training_forward_and_backward_are_exact(dev, name, R, S):
    """model(pts, viewdirs) and .backward() in every precision that trains the model: the training forward's raw, every
    bias gradient, every weight-gradient element outside the sin / cos columns, g_pts and g_viewdirs equal the float64
    reference element by element; training forward and inference forward agree bit for bit."""
    sd, pts, vd, g_raw, ref = case(name, R, S)
    m = gpu_model(dev, name)
    for precision in PRECISIONS[name]:
        tag = "%s %dx%d %s:" % (name, R, S, precision)
        m.precision = precision
        m.zero_grad(set_to_none=True)
        p = pts.to(dev).requires_grad_(True)
        v = vd.to(dev).requires_grad_(True) if vd is not None else None
        raw = m(p, v)
        assert raw.requires_grad
        (raw * g_raw.to(dev)).sum().backward()
        with torch.no_grad():
            inferred = m(pts.to(dev), vd.to(dev) if vd is not None else None)
        torch.cuda.synchronize()
        assert_exact(tag + " raw", raw, ref["raw"])
        assert_exact(tag + " inference raw", inferred, ref["raw"])
        assert torch.equal(inferred, raw.detach()), tag
        assert_param_grads(tag, named_grads(m), ref, precision)
        assert_exact(tag + " g_pts", p.grad, ref["g_pts"])
        if v is not None:
            assert_exact(tag + " g_viewdirs", v.grad, ref["g_vd"])
    forget(name, R, S)


@gpu
@pytest.mark.parametrize("name,R,S", RAYS_CASES)
def test_rays_mode_is_exact(dev, name, R, S):
    """forward_rays(rays, z_vals): the raw equals the points-mode raw at o + d z (the kernel's and the reference's), the
    parameter gradients are the points mode's, and g_rays is exact: dL/do = sum_s g_pts, dL/dd = sum_s z g_pts, zeros for
    near / far, dL/dviewdirs behind them -- accumulated with atomics, in any order, on integers and quarters."""
    rays, z, g_raw, pts, vd, ref, g_rays = rays_case(name, R, S)
    m = gpu_model(dev, name)
    for precision in PRECISIONS[name]:
        tag = "%s rays %dx%d %s:" % (name, R, S, precision)
        m.precision = precision
        m.zero_grad(set_to_none=True)
        r = rays.to(dev).requires_grad_(True)
        raw = m.forward_rays(r, z.to(dev))
        (raw * g_raw.to(dev)).sum().backward()
        with torch.no_grad():
            at_points = m(pts.to(dev), vd.to(dev) if vd is not None else None)
        torch.cuda.synchronize()
        assert_exact(tag + " raw", raw, ref["raw"])
        assert torch.equal(raw.detach(), at_points), tag
        assert_param_grads(tag, named_grads(m), ref, precision)
        assert_exact(tag + " g_rays", r.grad, g_rays)


def tiled_case(name, n_points):
    """A large inference batch at the cost of a small reference: the 41 x 97 case repeated along the ray axis (3977
    points per repeat, so the repeats do not line up with the 256-point tiles)."""
    sd, pts, vd, g_raw, ref = case(name, 41, 97)
    rays = -(-n_points // 97)
    reps = -(-rays // 41)
    return (pts.repeat(reps, 1, 1)[:rays], vd.repeat(reps, 1)[:rays] if vd is not None else None, ref["raw"].repeat(reps, 1, 1)[:rays])


@gpu
@pytest.mark.parametrize("name", sorted(ARCHS))
def test_inference_is_exact(dev, name):
    """Under torch.no_grad() (nerf_amd_nerf_forward) every network gives the reference's raw in every precision, at the
    awkward counts and, for the fused bf16 kernel, in both shapes of its weight pipeline (nerf_amd_set_tuning key 0: the
    continuous ring and the per-tile kernel), with one and with two tiles for some workgroups."""
    from nerf_shared_amd import _lib
    m = gpu_model(dev, name)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    batches = []
    for R, S in INFER_SIZES:
        sd, pts, vd, g_raw, ref = case(name, R, S)
        batches.append(("%dx%d" % (R, S), pts, vd, ref["raw"]))
    if name in FUSED or name in INFER_EXTRA:
        for n in (256 * n_cu + 300, 2 * 256 * n_cu + 513):
            batches.append(("%d points" % n,) + tiled_case(name, n))
    try:
        for precision in PRECISIONS[name]:
            m.precision = precision
            for variant in ((0, 41) if precision == "bf16" else (0,)):
                _lib.check(_lib.lib.nerf_amd_set_tuning(0, variant), "set_tuning")
                for what, pts, vd, want in batches:
                    with torch.no_grad():
                        raw = m(pts.to(dev), vd.to(dev) if vd is not None else None)
                    torch.cuda.synchronize()
                    assert_exact("%s %s %s variant %d: raw" % (name, what, precision, variant), raw, want)
    finally:
        _lib.lib.nerf_amd_set_tuning(0, 0)


@gpu
@pytest.mark.parametrize("name,P", EMBEDDED)
def test_mlp_on_embedded_rows_is_exact(dev, name, P):
    """NeRF.MLP on already-embedded integer rows (nerf_amd_mlp_embedded, the exact-fp32 kernel), weights on every column."""
    sd, x, raw, _, _ = embedded_case(name, P)
    m = gpu_model(dev, name, sd, "embedded")
    for precision in PRECISIONS[name]:          # (the kernel is the exact one whatever the model renders in)
        m.precision = precision
        assert_exact("%s MLP %s: raw" % (name, precision), m.MLP(x.to(dev)), raw)


ACCUMULATION = [(name, precision) for name in ("vd_10_4", "novd_out4", "d4_w128_skip2") for precision in PRECISIONS[name]]


@gpu
@pytest.mark.parametrize("name,precision", ACCUMULATION)
def test_two_backward_passes_accumulate_exactly(dev, name, precision):
    """Two backward passes into the same .grad without zero_grad: every .grad is exactly twice the reference (the
    kernels overwrite their own buffers, autograd accumulates).  No input requires grad here: the dX chain runs in the
    instantiation a training step uses, without the encoding products."""
    sd, pts, vd, g_raw, ref = case(name, 70, 13)
    m = gpu_model(dev, name)
    m.precision = precision
    for _ in range(2):
        raw = m(pts.to(dev), vd.to(dev) if vd is not None else None)
        (raw * g_raw.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert_param_grads("%s %s twice:" % (name, precision), named_grads(m), ref, precision, scale=2.0)


@gpu
@pytest.mark.parametrize("name,precision", ACCUMULATION)
def test_two_evaluations_in_one_graph_sum_exactly(dev, name, precision):
    """One model at two point sets inside one graph: the gradients are the exact sum of both (two saved workspaces alive
    at once, neither may leak into the other)."""
    a, b = case(name, 70, 13), case(name, 17, 241)
    m = gpu_model(dev, name)
    m.precision = precision
    loss = 0
    for sd, pts, vd, g_raw, ref in (a, b):
        loss = loss + (m(pts.to(dev), vd.to(dev) if vd is not None else None) * g_raw.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    ra, rb = a[4], b[4]
    both = dict(ra, grads={k: ra["grads"][k] + rb["grads"][k] for k in ra["grads"]},
                bf16_model={k: ra["bf16_model"][k] + rb["bf16_model"][k] for k in ra["bf16_model"]})
    assert_param_grads("%s %s two sets:" % (name, precision), named_grads(m), both, precision)


# ================================================================================================ partial packs
# nerf_amd_model_update_copies(copies, others_current = 1) packs the copies it is asked for and leaves every other copy
# alone.  All copies are packed from weights A, one bit is re-packed from other weights, and the kernel that reads that
# copy must give the other weights' reference while a kernel that reads another copy still gives A's.
#   B: other weights, A's biases.  C: A's weights, other biases (the 16-row bias table is read by the bf16 and the split
#   kernel, so either bit has to pack it).
# A backward copy is read after a forward from the matching forward copy, which still holds A: the dX chain then runs B's
# transposed weights over A's ReLU masks.  Its reference is the gradient of the network with B's weights whose ReLUs are
# replaced by A's recorded masks ("mixed").
PARTIAL = {"vd_10_4": ("BF16", "SPLIT", "FP32", "BWD", "BWD_SPLIT", "FP32_BWD", "BF16_FOLD"), "novd_out4": ("FP32", "FP32_BWD")}
PARTIAL_RS = (11, 3)          # 33 points: two 16-column tiles and a ragged one
# bit -> (precision of its consumer, precision of a consumer of another copy)
PARTIAL_FORWARD = {"BF16": ("bf16", "fp32_split"), "SPLIT": ("fp32_split", "bf16"), "FP32": ("fp32", "bf16")}
PARTIAL_BACKWARD = {"BWD": ("bf16", "fp32_split"), "BWD_SPLIT": ("fp32_split", "bf16"), "FP32_BWD": ("fp32", "bf16")}


def abi_names(arch):
    """Parameter tensors in the order of include/nerf_amd.h."""
    heads = ["feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"] if arch["use_viewdirs"] else ["output_linear"]
    return ["pts_linears.%d" % i for i in range(arch["D"])] + heads


def masked_input_grads(arch, sd_masks, sd, pts, vd, g_raw):
    """(g_pts, g_viewdirs, largest |dL/d pre-activation|) in float64 of the network with weights `sd` whose ReLUs are the
    masks that the network with weights `sd_masks` records at the same inputs."""
    A = _arch(arch)

    def encoded(p64, v64):
        e_dirs = O.embed(v64[:, None].expand(p64.shape).reshape(-1, 3), A.multires_views, A.i_embed) if v64 is not None else None
        return O.embed(p64.reshape(-1, 3), A.multires, A.i_embed), e_dirs

    tape = []
    with torch.no_grad():
        net64({k: v.double() for k, v in sd_masks.items()}, arch, *encoded(pts.double(), vd.double() if vd is not None else None), tape)
    masks = iter([(z > 0).double() for _, _, z, relu in tape if relu])
    p64 = pts.double().requires_grad_(True)
    v64 = vd.double().requires_grad_(True) if vd is not None else None
    tape = []
    raw = net64({k: v.double() for k, v in sd.items()}, arch, *encoded(p64, v64), tape, act=lambda z: z * next(masks))
    (raw.reshape(g_raw.shape) * g_raw.double()).sum().backward()
    return p64.grad.detach(), v64.grad.detach() if v64 is not None else None, max(float(z.grad.abs().max()) for _, _, z, _ in tape)


def partial_case(name):
    """Weights A, B, C, the inputs, the references of all three and the mixed dX references; computed once."""
    key = ("partial", name)
    if key not in _CACHE:
        arch = ARCHS[name]
        A = weights(name)
        other = integer_state_dict(arch, 900 + WEIGHT_SEED[name])
        B = {k: (A if k.endswith(".bias") else other)[k] for k in A}
        C = {k: (other if k.endswith(".bias") else A)[k] for k in A}
        pts, vd, g_raw = integer_inputs(arch, *PARTIAL_RS, 4242 + WEIGHT_SEED[name])
        refs = {tag: reference(arch, sd, pts, vd, g_raw) for tag, sd in (("A", A), ("B", B), ("C", C))}
        _CACHE[key] = (dict(A=A, B=B, C=C), pts, vd, g_raw, refs, masked_input_grads(arch, A, B, pts, vd, g_raw))
    return _CACHE[key]


@pytest.mark.parametrize("name", sorted(PARTIAL))
def test_partial_pack_generator_meets_the_preconditions(name):
    """Exactness is owed on all three weight sets and on the mixed dX chain; the three references differ from each other
    (a kernel that read the wrong copy cannot pass); with the same weights on both sides the mixed chain is the plain one."""
    arch = ARCHS[name]
    sds, pts, vd, g_raw, refs, (g_pts, g_vd, max_dx) = partial_case(name)
    assert pts.shape[0] * pts.shape[1] == 33
    for tag, sd in sds.items():
        assert all(is_integer(v) for v in sd.values())
        for k, m in sincos_columns(arch).items():
            assert float(sd[k][:, m].abs().max()) == 0.0, (tag, k)
        check_exactness_owed(arch, refs[tag])
    for n in abi_names(arch):
        assert torch.equal(sds["A"][n + ".bias"], sds["B"][n + ".bias"]) and not torch.equal(sds["A"][n + ".weight"], sds["B"][n + ".weight"])
        assert torch.equal(sds["A"][n + ".weight"], sds["C"][n + ".weight"])
        if sds["A"][n + ".bias"].numel() >= 16:           # (a head of one or three rows may draw the same biases twice)
            assert not torch.equal(sds["A"][n + ".bias"], sds["C"][n + ".bias"])
    for a, b in (("A", "B"), ("A", "C"), ("B", "C")):
        assert not torch.equal(refs[a]["raw"], refs[b]["raw"]), (a, b)
    assert is_integer(g_pts) and max_dx <= 256 and (g_vd is None or is_integer(g_vd))
    assert not torch.equal(g_pts, refs["A"]["g_pts"]) and not torch.equal(g_pts, refs["B"]["g_pts"])
    same = masked_input_grads(arch, sds["A"], sds["A"], pts, vd, g_raw)
    assert torch.equal(same[0], refs["A"]["g_pts"]) and (vd is None or torch.equal(same[1], refs["A"]["g_vd"]))
    if arch["use_viewdirs"]:           # the folded stream of B and C: W' and b' are exact too (test_gpu_fold.py)
        for tag in ("B", "C"):
            wf, bf = sds[tag]["feature_linear.weight"].double(), sds[tag]["feature_linear.bias"].double()
            wv, bv = sds[tag]["views_linears.0.weight"].double(), sds[tag]["views_linears.0.bias"].double()
            w, b = wv[:, :arch["W"]] @ wf, wv[:, :arch["W"]] @ bf + bv
            assert is_integer(w) and is_integer(b) and float(w.abs().max()) <= 256 and float(b.abs().max()) <= 256


class PackedModel:
    """A library model driven through the C ABI, so that the test decides which copy is packed from which weights."""

    def __init__(self, dev, arch):
        import ctypes
        from nerf_shared_amd import _lib
        self._lib, self.lib, self.dev, self.arch = _lib, _lib.lib, dev, arch
        self.ch = 4 if arch["use_viewdirs"] else arch["output_ch"]
        a = _lib.make_arch(arch["D"], arch["W"], arch["output_ch"], arch["skips"], arch["use_viewdirs"], arch["multires"],
                           arch["multires_views"], 0)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.nerf_amd_model_create(ctypes.byref(a), dev.index or 0, ctypes.byref(self.h)), "nerf_amd_model_create")
        self.stream = _lib.stream_of(dev)

    def close(self):
        torch.cuda.synchronize()
        self.lib.nerf_amd_model_destroy(self.h)

    def pack(self, sd, copies, others_current):
        import ctypes
        names = abi_names(self.arch)
        live = [sd[n + ".weight"].to(self.dev).contiguous() for n in names] + [sd[n + ".bias"].to(self.dev).contiguous() for n in names]
        n = len(names)
        wp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in live[:n]])
        bp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in live[n:]])
        self._lib.check(self.lib.nerf_amd_model_update_copies(self.h, wp, bp, n, copies, others_current, self.stream), "update_copies")
        torch.cuda.synchronize()          # (the parameter tensors die with this call)

    def forward(self, precision, pts, vd):
        R, S = pts.shape[:2]
        p, v = pts.to(self.dev).reshape(-1, 3).contiguous(), vd.to(self.dev).contiguous() if vd is not None else None
        out = torch.empty(R * S, self.ch, device=self.dev)
        self._lib.check(self.lib.nerf_amd_nerf_forward(self.h, p.data_ptr(), self._lib.ptr(v), R, S, out.data_ptr(), self.prec(precision),
                                                       self.stream), "nerf_amd_nerf_forward")
        torch.cuda.synchronize()
        return out.reshape(R, S, self.ch)

    def prec(self, precision):
        return {"bf16": self._lib.PREC_BF16, "fp32_split": self._lib.PREC_FP32_SPLIT, "fp32": self._lib.PREC_FP32}[precision]

    def forward_backward_inputs(self, precision, pts, vd, g_raw):
        """(raw, g_pts, g_viewdirs) of nerf_amd_field_forward_train followed by nerf_amd_field_backward_inputs."""
        R, S = pts.shape[:2]
        prec = self.prec(precision)
        p, v = pts.to(self.dev).reshape(-1, 3).contiguous(), vd.to(self.dev).contiguous() if vd is not None else None
        g = g_raw.to(self.dev).reshape(R * S, self.ch).contiguous()
        ws = torch.empty(max(self.lib.nerf_amd_train_workspace(self.h, R * S, prec), 1), dtype=torch.uint8, device=self.dev)
        raw, g_pts = torch.empty(R * S, self.ch, device=self.dev), torch.empty(R * S, 3, device=self.dev)
        g_vd = torch.zeros(R, 3, device=self.dev) if v is not None else None
        self._lib.check(self.lib.nerf_amd_field_forward_train(self.h, p.data_ptr(), self._lib.ptr(v), None, 0, None, R, S, raw.data_ptr(),
                                                              ws.data_ptr(), ws.numel(), prec, self.stream), "nerf_amd_field_forward_train")
        self._lib.check(self.lib.nerf_amd_field_backward_inputs(self.h, g.data_ptr(), p.data_ptr(), self._lib.ptr(v), None, 0, None, R, S,
                                                                ws.data_ptr(), ws.numel(), g_pts.data_ptr(), None, self._lib.ptr(g_vd), prec,
                                                                self.stream), "nerf_amd_field_backward_inputs")
        torch.cuda.synchronize()
        return raw.reshape(R, S, self.ch), g_pts.reshape(R, S, 3), g_vd


@gpu
@pytest.mark.parametrize("name", sorted(PARTIAL))
def test_a_partial_pack_packs_what_is_asked_for_and_nothing_else(dev, name):
    """Every copy from A, then one NERF_AMD_COPY_* bit from B with others_current = 1: the copy's consumer gives B's
    reference (a backward copy: the mixed one) and a consumer of another copy still gives A's, both bit for bit.  Then the
    16-row bias table: packing the split copy alone, or the bf16 copy alone, from C carries C's biases into that kernel."""
    from nerf_shared_amd import _lib
    sds, pts, vd, g_raw, refs, (mixed_g_pts, mixed_g_vd, _) = partial_case(name)
    everything = _lib.COPY_ALL | (_lib.COPY_BF16_FOLD if ARCHS[name]["use_viewdirs"] else 0)
    m = PackedModel(dev, ARCHS[name])
    try:
        for bit in PARTIAL[name]:
            tag = "%s, %s from B:" % (name, bit)
            m.pack(sds["A"], everything, 0)
            m.pack(sds["B"], getattr(_lib, "COPY_" + bit), 1)
            if bit in PARTIAL_FORWARD:
                mine, other = PARTIAL_FORWARD[bit]
                assert_exact("%s %s raw" % (tag, mine), m.forward(mine, pts, vd), refs["B"]["raw"])
                assert_exact("%s %s raw (another copy)" % (tag, other), m.forward(other, pts, vd), refs["A"]["raw"])
            elif bit in PARTIAL_BACKWARD:
                mine, other = PARTIAL_BACKWARD[bit]
                raw, g_pts, g_vd = m.forward_backward_inputs(mine, pts, vd, g_raw)
                assert_exact("%s %s raw (the forward copy)" % (tag, mine), raw, refs["A"]["raw"])
                assert_exact("%s %s g_pts" % (tag, mine), g_pts, mixed_g_pts)
                if vd is not None:
                    assert_exact("%s %s g_viewdirs" % (tag, mine), g_vd, mixed_g_vd)
                raw, g_pts, g_vd = m.forward_backward_inputs(other, pts, vd, g_raw)
                assert_exact("%s %s g_pts (another copy)" % (tag, other), g_pts, refs["A"]["g_pts"])
                if vd is not None:
                    assert_exact("%s %s g_viewdirs (another copy)" % (tag, other), g_vd, refs["A"]["g_vd"])
            else:                        # the folded stream: nerf_amd_nerf_forward reads it under tuning key 2 = 2
                assert_exact("%s unfolded bf16 raw (another copy)" % tag, m.forward("bf16", pts, vd), refs["A"]["raw"])
                try:
                    _lib.check(_lib.lib.nerf_amd_set_tuning(2, 2), "set_tuning")
                    assert_exact("%s folded bf16 raw" % tag, m.forward("bf16", pts, vd), refs["B"]["raw"])
                finally:
                    _lib.lib.nerf_amd_set_tuning(2, 0)
        if name in FUSED and "BF16" in PARTIAL[name]:
            for bit, precision in (("SPLIT", "fp32_split"), ("BF16", "bf16")):
                m.pack(sds["A"], everything, 0)
                m.pack(sds["C"], getattr(_lib, "COPY_" + bit), 1)
                assert_exact("%s, %s from C: %s raw" % (name, bit, precision), m.forward(precision, pts, vd), refs["C"]["raw"])
    finally:
        m.close()
