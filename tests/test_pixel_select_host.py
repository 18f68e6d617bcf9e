"""CPU tests of the pixel-selection surface (nerf_amd_draw_pixels, nerf_amd_interest_points, nerf_amd_dilate_mask,
nerf_amd_compact_mask; utils.PixelSampler): the bindings agree with the header, the DRAW AS DEFINED (evaluated by the numpy
mirror, tests/pixel_select_mirror.py) is a uniform sample without replacement by three statistical conditions with bounds
from the chi-square and hypergeometric distributions, the mirror's dilation is scipy's, and the refusals that need no
device.  No compute call reaches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from nerf_shared_amd import _lib, utils  # noqa: E402
import pixel_select_mirror as mirror  # noqa: E402

NEW_SYMBOLS = ("nerf_amd_draw_pixels", "nerf_amd_interest_points", "nerf_amd_dilate_mask", "nerf_amd_compact_mask",
               "nerf_amd_interest_points_workspace")


def _declared_argument_counts():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    counts = {}
    for name, args in re.findall(r"\b(nerf_amd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    return counts


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_entry_points_are_bound_as_the_header_declares_them(name):
    declared = _declared_argument_counts()
    assert name in _lib.EXPORTS
    assert name in declared, "include/nerf_amd.h does not declare %s" % name
    fn = getattr(_lib.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name], (name, len(fn.argtypes or ()), declared[name])
    assert len(getattr(_lib.lib, "nerf_amd_rays_at_pixels").argtypes) == declared["nerf_amd_rays_at_pixels"]      # the parser reads the header


# ------------------------------------------------------------------------------------------------ the draw as defined
SEED, DRAWS = 1234, 4000
_DRAWN = {}


def drawn(M, n):
    """Mirror draws 0..DRAWS-1 at SEED, int64 [DRAWS, n]; computed once per (M, n)."""
    if (M, n) not in _DRAWN:
        _DRAWN[(M, n)] = np.stack([mirror.draw_indices(M, n, SEED, d) for d in range(DRAWS)], 0)
    return _DRAWN[(M, n)]


def test_mix_is_the_stated_function():
    """The mirror's vectorised mix against the five statements of the definition in Python integers."""
    def mix(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
        return x
    xs = [0, 1, 2, 0x9e3779b9, 0xffffffff, 0x80000000, 123456789]
    assert [int(v) for v in mirror.mix(np.array(xs, dtype=np.uint64))] == [mix(x) for x in xs]
    assert [mirror.half_bits(M) for M in (1, 2, 3, 4, 5, 16, 17, 37, 1000, 4097, 160000)] == [1, 1, 1, 1, 2, 2, 3, 3, 5, 7, 9]


@pytest.mark.parametrize("M,n", [(1000, 64), (37, 16)])
def test_draws_are_distinct_uniform_and_independent(M, n):
    """4000 draws at one seed.  (a) every draw is n distinct indices below M.  (b) Pearson chi-square of how often each index
    was drawn against D n / M, without a finite-population correction (which only makes the test stricter): at most
    nu + 6 sqrt(2 nu), nu = M - 1, the mean of chi-square_nu plus six standard deviations.  (c) the same for slot 0 alone
    against D / M.  (d) the mean overlap of consecutive draws within six standard errors of the hypergeometric mean n^2 / M
    (variance n (n/M) (1 - n/M) (M - n) / (M - 1) per pair).  The seed is fixed: the outcome is deterministic."""
    d = drawn(M, n)
    assert d.shape == (DRAWS, n) and d.min() >= 0 and d.max() < M
    assert all(len(set(row)) == n for row in d.tolist())                                                    # (a)
    nu = M - 1
    bound = nu + 6 * np.sqrt(2 * nu)
    counts = np.bincount(d.ravel(), minlength=M).astype(np.float64)
    exp = DRAWS * n / M
    chi_all = float(((counts - exp) ** 2 / exp).sum())
    counts0 = np.bincount(d[:, 0], minlength=M).astype(np.float64)
    exp0 = DRAWS / M
    chi_0 = float(((counts0 - exp0) ** 2 / exp0).sum())
    overlap = np.array([len(np.intersect1d(d[k], d[k + 1])) for k in range(DRAWS - 1)], dtype=np.float64)
    mean_h = n * n / M
    var_h = n * (n / M) * (1 - n / M) * (M - n) / (M - 1)
    se = np.sqrt(var_h / (DRAWS - 1))
    print("M %d n %d: chi2 all %.1f, slot 0 %.1f (bound %.1f); overlap %.4f, expected %.4f +- %.4f"
          % (M, n, chi_all, chi_0, bound, overlap.mean(), mean_h, se))
    assert chi_all <= bound                                                                                 # (b)
    assert chi_0 <= bound                                                                                   # (c)
    assert abs(overlap.mean() - mean_h) <= 6 * se                                                           # (d)


@pytest.mark.parametrize("M", [5, 1])
def test_a_full_draw_is_a_permutation(M):
    for d in range(200):
        assert sorted(mirror.draw_indices(M, M, SEED, d).tolist()) == list(range(M))


def test_the_key_uses_the_low_32_bits_of_the_counter():
    assert np.array_equal(mirror.draw_indices(1000, 64, 7, 2 ** 32), mirror.draw_indices(1000, 64, 7, 0))
    assert not np.array_equal(mirror.draw_indices(1000, 64, 7, 2 ** 32 - 1), mirror.draw_indices(1000, 64, 7, 0))


# ------------------------------------------------------------------------------------------------ dilation
@pytest.mark.parametrize("I", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_mirror_dilation_is_scipys_grey_dilation(k, I):
    """cv2.dilate's window for a k x k kernel is [-a, k - 1 - a], a = k // 2.  scipy's grey_dilation with a k x k footprint has
    that window for odd k and, for even k, with origin = -1 (its default puts the longer side of an even window the other
    way); mode='constant', cval=0: off-image pixels never win.  One iteration is also checked against the definition
    written out pixel by pixel, so the origin is not taken on trust."""
    ndimage = pytest.importorskip("scipy.ndimage")
    m = np.zeros((9, 13), np.uint8)
    m[0, 0] = m[0, 12] = m[8, 0] = m[8, 12] = m[4, 6] = 1
    ref = m
    for _ in range(I):
        ref = ndimage.grey_dilation(ref, footprint=np.ones((k, k)), mode="constant", cval=0, origin=0 if k % 2 else -1)
    by_hand = np.zeros_like(m)                                  # the definition, literally, for one iteration
    a = k // 2
    for y in range(9):
        for x in range(13):
            win = m[max(0, y - a):min(9, y + k - a), max(0, x - a):min(13, x + k - a)]
            by_hand[y, x] = win.max()
    assert np.array_equal(mirror.dilate(m, k, 1), by_hand)
    assert np.array_equal(mirror.dilate(m, k, I), ref)


# ------------------------------------------------------------------------------------------------ refusals without a device
def test_host_side_refusals():
    img = np.zeros((6, 8, 3), np.uint8)
    with pytest.raises(_lib.NerfAmdError, match="strategy"):
        utils.PixelSampler(img, 4, strategy="sift")
    for bad in ([[8, 0]], [[0, 6]], [[-1, 2]], torch.tensor([[3, 3], [0, 6]])):
        with pytest.raises(_lib.NerfAmdError, match="outside"):
            utils.PixelSampler(img, 1, strategy="interest_point", points=bad)
    for shape in ((6, 8), (6, 8, 2), (6, 8, 5), (1, 6, 8, 3)):
        with pytest.raises(_lib.NerfAmdError, match=r"\[H, W, 3\]"):
            utils.PixelSampler(np.zeros(shape, np.uint8), 1, strategy="random")
        with pytest.raises(_lib.NerfAmdError, match=r"\[H, W, 3\]"):
            utils.find_POI(np.zeros(shape, np.uint8))
    with pytest.raises(_lib.NerfAmdError, match="uint8"):
        utils.PixelSampler(np.zeros((6, 8, 3), np.int32), 1, strategy="random")
