"""numpy restatement of the split form of dconv_fwd_kernel (csrc/dconv.h, FMT != 0): the LDS image and the arithmetic the kernel is
to implement, for a 5x5 stride-2 layer of 16 -> 8 channels whose output grid is 8 x 16 (one tile, eight 16-pixel row blocks).

  LDS item    16 bytes = four consecutive k of one row.  Exact f32: [4 x f32].  Split: [4 x hi | 4 x lo] 16-bit terms -- the same
              footprint, so the tile's pixel stride CIP (dc_cip), the tab[] byte offsets and the filter image
              W4[slot * CIK / 4 + kq][n][.] are those of the f32 kernel.
  K order     lane (l15, kg) of a wave supplies k = 16 * chunk + 4 * kg + t, t = 0..3, for A and B alike: one 16-byte read per
              fragment, whose low half is the hi operand and whose high half the lo operand of a 16x16x16 16-bit MFMA.
  terms       w_lo x_hi + w_hi x_lo + w_hi x_hi per chunk (small terms first), f32 accumulators.
  rescale     2^(-2 EXP) in front of the epilogue for fp16 * 2^EXP; none for bf16.

The emulation accumulates in float64 (as tests/_fp16_split.py does: it states the FORMAT's error, not the matrix cores' summation
order) and is held to the per-product bounds that file's formats give: bf16 2^-16, fp16 * 2^6 2^-22 of sum |x| |w| per output."""
import numpy as np
import pytest

from tests import _fp16_split as fs

CI, N, S, PAD = 16, 8, 2, 1              # TF SAME, 5x5 stride 2: pad_before = (5 - 2) // 2
HO, WO = 8, 16                           # output grid = one tile TH x TW
HI, WI = S * HO, S * WO
CIK, NP = 16, 16                         # channel class of the instantiation; filter columns padded to a 16-wide block
IH, IW = S * (HO - 1) + 5, S * (WO - 1) + 5


def dc_cip(cik, s):
    return 4 if cik == 4 else (8 if s == 1 else 12) if cik == 8 else cik + (8 if s == 1 else 4)


CIP = dc_cip(CIK, S)                     # floats per tile pixel in LDS


def bits16(fmt, x, exp):
    """f32 array -> (hi, lo) uint16 bit patterns of the format's two terms."""
    if fmt == "bf16":
        hi, lo = fs.split_bf16(x)
        return (hi.view(np.uint32) >> 16).astype(np.uint16), (lo.view(np.uint32) >> 16).astype(np.uint16)
    hi, lo = fs.split(x, exp)
    return hi.view(np.uint16), lo.view(np.uint16)


def value16(fmt, u):
    u = np.ascontiguousarray(u, np.uint16)
    if fmt == "bf16":
        return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return u.view(np.float16).astype(np.float64)


def items(fmt, x4, exp):
    """[..., 4] f32 -> [..., 8] uint16: the 16-byte item [4 x hi | 4 x lo]."""
    hi, lo = bits16(fmt, x4, exp)
    return np.concatenate([hi, lo], axis=-1)


def lds_tile(fmt, x, exp):
    """The input halo tile as bytes: pixel (iy, ix) of the tile at (iy * IW + ix) * CIP * 4, its k-quad kq 16 * kq bytes further; zeros
    outside the image (the split of 0 is 0 in both formats)."""
    t = np.zeros((IH, IW, CIP * 2), np.uint16)          # CIP floats = 2 CIP 16-bit words per pixel
    xp = np.zeros((IH, IW, CI), np.float32)
    y0, x0 = -PAD, -PAD
    ys, xs = np.arange(IH) + y0, np.arange(IW) + x0
    oky, okx = (ys >= 0) & (ys < HI), (xs >= 0) & (xs < WI)
    xp[np.ix_(oky, okx)] = x[np.ix_(ys[oky], xs[okx])]
    t[:, :, :CI * 2] = items(fmt, xp.reshape(IH, IW, CI // 4, 4), exp).reshape(IH, IW, CI * 2)
    return t.reshape(-1).view(np.uint8)


def lds_filter(fmt, w, exp):
    """W4[slot * CIK / 4 + kq][n][item]: the packed image wp[slot][k / 4][n][k & 3] (f32, zero columns n >= N), split on its way in."""
    wp = np.zeros((25, CIK // 4, NP, 4), np.float32)
    wp[:, :, :N, :] = w.reshape(25, CI // 4, 4, N).transpose(0, 1, 3, 2)
    return items(fmt, wp, exp).reshape(-1).view(np.uint8)


def run_kernel(fmt, x, w, exp):
    """The MFMA loop of one tile, lane by lane: out[pixel][n] in f32."""
    tile, w4 = lds_tile(fmt, x, exp), lds_filter(fmt, w, exp)
    l15, kg = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")            # the 64 lanes of a wave
    out = np.zeros((HO, WO, NP), np.float64)

    def read_b128(buf, addr):                            # one 16-byte read per lane -> [16, 4, 8] 16-bit words
        assert (addr % 16 == 0).all() and addr.max() + 16 <= buf.size
        idx = addr[..., None] + np.arange(16)
        return buf[idx].reshape(16, 4, 16).view(np.uint16)

    nchunks = 25 * CIK // 16
    for ty in range(HO):                                 # row block rb = (ty, 16 pixels): TW = 16
        abase = ((S * ty) * IW + S * l15) * CIP * 4
        acc = np.zeros((NP, 16), np.float64)             # D^T: rows = channels, columns = pixels
        for g in range(nchunks):
            k16 = 16 * g + 4 * kg                        # first k of the lane's group: k = 16 * chunk + 4 * kg + t
            tap, kin = k16 // CIK, k16 % CIK
            tab = (((tap // 5) * IW + tap % 5) * CIP + kin) * 4
            xf = read_b128(tile, abase + tab)                                     # [pixel l15][kg][hi 0..3 | lo 4..7]
            wf = read_b128(w4, ((4 * g + kg) * NP + l15) * 16)                    # [column l15][kg][hi | lo]
            xh, xl = value16(fmt, xf[..., :4]), value16(fmt, xf[..., 4:])
            wh, wl = value16(fmt, wf[..., :4]), value16(fmt, wf[..., 4:])
            for a, b in ((wl, xh), (wh, xl), (wh, xh)):  # small terms first
                acc += np.einsum("nkj,pkj->np", a, b)
        out[ty] = acc.T
    if fmt == "fp16":
        out *= 2.0 ** (-2 * exp)
    return out[:, :, :N].astype(np.float32)


def im2col(x):
    xp = np.zeros((HI + 4, WI + 4, CI), np.float64)
    xp[PAD:PAD + HI, PAD:PAD + WI] = x
    cols = np.empty((HO, WO, 25, CI), np.float64)
    for ky in range(5):
        for kx in range(5):
            cols[:, :, ky * 5 + kx] = xp[ky:ky + S * HO:S, kx:kx + S * WO:S]
    return cols.reshape(HO * WO, 25 * CI)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((HI, WI, CI)).astype(np.float32)
    w = (rng.standard_normal((25, CI, N)) * 0.1).astype(np.float32)
    cols = im2col(x)
    exact = cols @ w.reshape(25 * CI, N).astype(np.float64)
    mag = np.abs(cols) @ np.abs(w.reshape(25 * CI, N)).astype(np.float64)
    return x, w, cols, exact, mag


def test_item_keeps_the_f32_footprint():
    """[4 hi | 4 lo] is 16 bytes like [4 x f32]: same CIP, same tab[] offsets, same filter image size."""
    v = np.arange(8, dtype=np.float32).reshape(2, 4)
    for fmt in ("bf16", "fp16"):
        it = items(fmt, v, fs.EXP)
        assert it.shape == (2, 8) and it.dtype == np.uint16 and it.nbytes == v.nbytes
    assert (S * CIP) % 16 == 8               # dc_cip's bank condition for the fragment reads is untouched


@pytest.mark.parametrize("fmt,per_product", [("bf16", 2.0 ** -16), ("fp16", 2.0 ** -22)])
def test_split_direct_conv_matches_the_format(case, fmt, per_product):
    x, w, cols, exact, mag = case
    got = run_kernel(fmt, x, w, fs.EXP).reshape(HO * WO, N).astype(np.float64)
    # the three terms and the rescale are the format's: the im2col product in tests/_fp16_split.py's statement of it
    ref = fs.matmul3_bf16(cols.astype(np.float32), w.reshape(25 * CI, N)) if fmt == "bf16" else fs.matmul3(cols.astype(np.float32), w.reshape(25 * CI, N))
    assert np.abs(got - ref).max() <= 2.0 ** -22 * np.abs(ref).max()              # f32 rounding of two float64 summation orders
    # ... and within the per-product bound of the format (the dropped lo * lo term and the lo terms' rounding), plus the final f32 rounding
    err = np.abs(got - exact)
    assert (err <= per_product * mag + 2.0 ** -23 * np.abs(exact)).all(), float((err / mag).max())
    # one term alone would miss that bound: the split is live
    hi_only = (fs.split_bf16(cols.astype(np.float32))[0].astype(np.float64) @ fs.split_bf16(w.reshape(25 * CI, N))[0].astype(np.float64)) if fmt == "bf16" else None
    if hi_only is not None:
        assert (np.abs(hi_only - exact) > per_product * mag).any()


def test_fp16_operand_scale_is_exact_and_removed():
    """x * 2^6 and the 2^-12 rescale are exact: a layer of small integers comes out exactly."""
    rng = np.random.default_rng(1)
    x = rng.integers(-3, 4, (HI, WI, CI)).astype(np.float32)
    w = rng.integers(-2, 3, (25, CI, N)).astype(np.float32)
    exact = im2col(x) @ w.reshape(25 * CI, N).astype(np.float64)
    for fmt in ("bf16", "fp16"):
        got = run_kernel(fmt, x, w, fs.EXP).reshape(HO * WO, N)
        np.testing.assert_array_equal(got, exact.astype(np.float32))
