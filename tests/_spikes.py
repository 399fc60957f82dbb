"""Cases with ONE dominant region per operand, for precision="fp16x3d" (tests/test_gpu_fp16x3d_ranges.py runs them on the device,
tests/test_fp16x3d_spike_cases.py checks the cases themselves against the float64 oracle and the numpy emulation).

The mode takes one power-of-two scale per operand from the operand's largest magnitude over the floats the loader STATES it reads
(csrc/igemm.h: ranges; csrc/dconv.hip: rx / rw; the split branches of csrc/cnn.cpp).  The largest entry is placed in [2^14, 2^15):
an element that the statement misses and that is more than ~2-4 x larger than the stated maximum leaves fp16 and the product is
inf / NaN.  Dense i.i.d. data cannot show that (every sub-range has the same maximum); a case here gives ONE image, ONE skip source,
ONE tap or ONE channel slice of an operand a magnitude that is at least DOMINANCE times the rest of it.

  pixel spikes   one pixel (all three channels) of one f32 frame set to +-2^K_PIXEL
  filter pokes   one filter element times 2^K_FILTER
K_PIXEL and K_FILTER are the two chosen constants.  Their lower end is the blindness guard (DOMINANCE = 8 for every operand a case
names, asserted from the oracle's cache); their upper end is RATIO_MAX: up to that ratio the emulation keeps the un-spiked rows of a
product f32-grade (the spiked entries push the others down towards the fp16 subnormal floor, include/ctxtrans.h), so a correct
implementation holds the bar of tests/test_gpu_fp16x3d.py on these cases."""
import numpy as np

from oracle import ctx_oracle as o

K_PIXEL = 14
K_FILTER = 14
DOMINANCE = 8.0
RATIO_MAX = 2.0 ** 15

# (H, W, d, F, B) of ContextSkipNew and the route the shape is there for
IMAGE_MAJOR = [(16, 16, 32, 32, 3), (16, 48, 32, 128, 3)]       # image-major loaders, odd B, non-square (and no power-of-two grid: the plain filter gradient)
POSITION_MAJOR = [(16, 16, 32, 32, 64), (32, 16, 32, 64, 32)]   # ...Q loaders from 64 images per launch, the rectangle-ordered ...R filter gradient
PATCH = [(32, 32, 32, 64, 5)]                                   # power-of-two grids below 64 images: the patch loaders ...P
SHAPES = IMAGE_MAJOR + POSITION_MAJOR + PATCH
REPLAY = (16, 48, 32, 128, 25)                                  # translate / encode at 25 frames: captured on the second call, then replayed


# ---------------------------------------------------------------------------------------------- pixel spikes
def pixel_cases(H, W, B, inputs=("src", "ctx", "tgt")):
    """(input, image, (y, x), sign): first and last image, first and last pixel; + at (0,0), - at (H-1,W-1)."""
    return [(which, n, pix, sign) for which in inputs for n in sorted({0, B - 1}) for pix, sign in (((0, 0), 1.0), ((H - 1, W - 1), -1.0))]


def spike(frames, which, n, pix, sign, k=K_PIXEL):
    """Copies of the f32 frames (src, ctx, tgt) with one pixel of one frame set to sign * 2^k."""
    out = [np.array(x, np.float32) for x in frames]
    out["src ctx tgt".split().index(which)][n, pix[0], pix[1], :] = np.float32(sign * 2.0 ** k)
    return out


def operands(c):
    """{name: the tensors of one split operand, stacked along images} from the cache of ctx_oracle.forward: the activation (A) side of
    every forward product and the seed of the backward.  The stacked `conv` encoder reads [tgt | src]; a decoder layer reads
    [decoder | ctx skip] for both passes (d1_cats / d2_cats hold the concats)."""
    ops = {}
    for sc, arrs in (("conv", ("e_tgt", "e_src")), ("conv_context", ("e_ctx",))):
        for k in range(1, 4):
            ops[f"{sc}/h{k}_conv x"] = [c[a][k - 1] for a in arrs]
        ops[f"{sc}/h4_lin x"] = [c[a][3] for a in arrs]
        ops[f"{sc}/hz_lin x"] = [c[a][4] for a in arrs]
    ops["translate/trans_h0 x"] = [c["tcat"]]
    ops["deconv/d_h0_lin x"] = [c["trans_z"], c["e_tgt"][5]]
    for k in range(1, 5):
        ops[f"deconv/d_h{k} x"] = [c["d1_cats"][k - 1], c["d2_cats"][k - 1]]
    ops["d loss / d out"] = [c["d1"][4] - c["tgt"], c["d2"][4] - c["tgt"]]
    return ops


# the operands a spike in each input is meant to dominate (image n of each against every other image of it)
NAMED = {
    "src": [f"conv/h{k}_conv x" for k in (1, 2, 3)] + ["conv/h4_lin x", "conv/hz_lin x", "translate/trans_h0 x"],
    "ctx": [f"conv_context/h{k}_conv x" for k in (1, 2, 3)] + ["conv_context/h4_lin x", "conv_context/hz_lin x", "translate/trans_h0 x"] +
           [f"deconv/d_h{k} x" for k in (1, 2, 3, 4)] + ["d loss / d out"],
    "tgt": [f"conv/h{k}_conv x" for k in (1, 2, 3)] + ["conv/h4_lin x", "conv/hz_lin x", "deconv/d_h0_lin x", "d loss / d out"],
}


def dominance(arrs, n):
    """Largest magnitude of image n of the operand over the largest magnitude of its other images."""
    region = max(float(np.abs(a[n]).max()) for a in arrs)
    rest = max(float(np.abs(np.delete(a, n, axis=0)).max()) for a in arrs)
    return region / rest


# ---------------------------------------------------------------------------------------------- filter pokes
TAPS = ((0, 0), (2, 2), (4, 4))


def tap_reached(k, nbig, nsmall, K=5, s=2, pad=1):
    """TF SAME, kernel 5, stride 2, even input: output position i reads input 2 i + k - 1.  True where some position lands inside."""
    return any(0 <= s * i + k - pad < nbig for i in range(nsmall))


def filter_layers(H, W, B, d_h4=False):
    """{filter name: (kind, big grid, small grid, images per launch)} of every filter that is an operand of a split product."""
    L = {}
    for sc, nimg in (("conv", 2 * B), ("conv_context", B)):
        for k in (1, 2, 3):
            L[f"{sc}/h{k}_conv/w"] = ("conv", (H >> k, W >> k), (H >> (k + 1), W >> (k + 1)), nimg)
        L[f"{sc}/h4_lin/Matrix"] = L[f"{sc}/hz_lin/Matrix"] = ("fc", None, None, nimg)
    for k in (1, 2, 3) + ((4,) if d_h4 else ()):
        L[f"deconv/d_h{k}/w"] = ("deconv", (H >> (4 - k), W >> (4 - k)), (H >> (5 - k), W >> (5 - k)), 2 * B)
    for n in ("translate/trans_h0/Matrix", "translate/trans_z/Matrix", "deconv/d_h0_lin/Matrix"):
        L[n] = ("fc", None, None, B)
    return L


def filter_cases(name, shape, layer):
    """[(index, reached)]: taps (0,0), (2,2), (4,4) x channels (0,0), (last,last) of a conv filter; the four corners of an FC matrix."""
    kind, big, small, _ = layer
    if kind == "fc":
        return [((i, j), True) for i in (0, shape[0] - 1) for j in (0, shape[1] - 1)]
    out = []
    for ky, kx in TAPS:
        reached = tap_reached(ky, big[0], small[0]) and tap_reached(kx, big[1], small[1])
        out += [((ky, kx, a, b), reached) for a, b in ((0, 0), (shape[2] - 1, shape[3] - 1))]
    return out


def poke(p, name, idx, factor=2.0 ** K_FILTER):
    """A copy of the parameter tree with one element of one filter multiplied by `factor` (a power of two, or inf)."""
    q = dict(p)
    q[name] = p[name].copy()
    q[name][idx] = q[name][idx] * factor if np.isfinite(factor) else factor
    return q


def poke_dominance(w, idx, factor=2.0 ** K_FILTER):
    rest = np.abs(w).copy()
    rest[idx] = 0.0
    return float(abs(w[idx]) * factor / rest.max())


# ---------------------------------------------------------------------------------------------- exponent edges of split_absmax
def with_max(w, target):
    """w rescaled by a power of two and its largest-magnitude entry set to +-target exactly: the operand's maximum IS target."""
    w = np.array(w, np.float32)
    i = np.unravel_index(np.abs(w).argmax(), w.shape)
    e = int(np.floor(np.log2(float(target)))) - int(np.floor(np.log2(float(abs(w[i]))))) - 1     # every other entry ends up below target / 2 ... target
    w = w * np.float32(2.0 ** e)
    assert np.abs(w).max() < abs(float(target))
    w[i] = np.float32(np.sign(w[i]) * target)
    return w


def no_bias(p):
    return {n: (np.zeros_like(v) if n.endswith("bias") or n.endswith("biases") else v.copy()) for n, v in p.items()}


def exponent_edge_cases(p, m_pos=3, m_neg=-9):
    """{case: (parameter tree without biases, {filter: expected exponent e of tests/_fp16_dyn.exponent})}.  Only the `conv` encoder is
    touched: its h1 output feeds h2 alone, so a compensating pair leaves everything behind h2 at its usual size (conv_context's h1
    output is also the decoder's skip)."""
    p = no_bias(p)
    f32 = {n: np.asarray(v, np.float32) for n, v in p.items()}
    cases = {}

    def scaled(h1, h2=None):
        q = dict(f32)
        q["conv/h1_conv/w"] = h1(f32["conv/h1_conv/w"])
        if h2:
            q["conv/h2_conv/w"] = h2(f32["conv/h2_conv/w"])
        return q

    for m in (m_pos, m_neg):
        top = np.float32(2.0 ** m)
        cases[f"max = 2^{m}"] = (scaled(lambda w: with_max(w, top)), {"conv/h1_conv/w": 14 - m})
        cases[f"max = 2^{m} - 1 ulp"] = (scaled(lambda w: with_max(w, np.nextafter(top, np.float32(0)))), {"conv/h1_conv/w": 14 - (m - 1)})
    e1, e2 = (fd_exponent(f32[f"conv/h{k}_conv/w"]) for k in (1, 2))
    cases["h1 x 2^100, h2 x 2^-100"] = (scaled(lambda w: w * np.float32(2.0 ** 100), lambda w: w * np.float32(2.0 ** -100)),
                                        {"conv/h1_conv/w": e1 - 100, "conv/h2_conv/w": e2 + 100})
    cases["h1 x 2^-115, h2 x 2^115"] = (scaled(lambda w: w * np.float32(2.0 ** -115), lambda w: w * np.float32(2.0 ** 115)),
                                        {"conv/h1_conv/w": 126, "conv/h2_conv/w": e2 - 115})          # absmax < 2^-112: the clamp binds
    return cases


def subnormal_filter(p):
    """`conv/h1_conv/w` all zero but one f32 subnormal entry (2^-140) at the centre tap."""
    q = {n: np.asarray(v, np.float32) for n, v in no_bias(p).items()}
    w = np.zeros_like(q["conv/h1_conv/w"])
    w[2, 2, 5, 7] = np.float32(2.0 ** -140)
    q["conv/h1_conv/w"] = w
    return q


def fd_exponent(x):
    from tests import _fp16_dyn as fd
    return fd.exponent(x)


def f64_frames(frames):
    return [np.asarray(x, np.float32).astype(np.float64) for x in frames]


def base_frames(fr_u8):
    return [o.preprocess_u8(x) for x in fr_u8]


# ---------------------------------------------------------------------------------------------- the other engines
def real_case(H, W, B):
    from tests.test_gpu_real import make
    cfg, p, fr = make(H, W, B, seed=9)
    return cfg, p, base_frames(fr)


def real_pixel_cases(H, W, B):
    """First and last image; the three inputs; both corner pixels."""
    return [("src", 0, (0, 0), 1.0), ("ctx", B - 1, (H - 1, W - 1), -1.0), ("tgt", B - 1, (0, 0), 1.0), ("ctx", 0, (0, 0), 1.0)]


def real_filter_pokes(p):
    """One poke in a conv filter, one in each kind of transposed conv (d_h2 is stride 1, d_h1 stride 2): last tap / last channels, first
    tap / last channels, centre tap / first channels."""
    out = []
    for name, idx in (("conv/h2_conv/w", (4, 4, -1, -1)), ("deconv/d_h2/w", (0, 0, -1, -1)), ("deconv/d_h1/w", (2, 2, 0, 0))):
        out.append((name, tuple(i % s for i, s in zip(idx, p[name].shape))))
    return out


INCEP2 = (2, 2, 128, 8, 128)          # H, W, C, d, F of ContextAEInception2's test shape


def incep2_case(B):
    from tests.test_gpu_incep import make
    H, W, C, d, F = INCEP2
    return make(H, W, C, d, F, B, seed=2)


def incep2_pixel_cases(B):
    """Feature maps, not frames: spike() sets every channel of one position of one map."""
    return [("src", 0, (0, 0), 1.0), ("ctx", B - 1, (1, 1), 1.0), ("tgt", B - 1, (0, 0), 1.0), ("ctx", 0, (0, 0), 1.0)]


def incep2_filter_pokes(p):
    """The centre tap (reached on every grid, 1x1 included) of an encoder filter and of a stride-1 transposed filter, last channels."""
    return [(name, (1, 1, p[name].shape[2] - 1, p[name].shape[3] - 1)) for name in ("conv/h1_conv/w", "deconv/d_h3/w")]


def stacked_dominance(c, which, n, layers=(0, 1, 2)):
    """The table-driven engines run ONE stacked encoder pass over [tgt | src | ctx]: dominance of image n of input `which` in the
    activations e[k] that the next layer reads, against every other image of all three."""
    out = []
    for k in layers:
        arrs = [c["e_tgt"][k], c["e_src"][k], c["e_ctx"][k]]
        region = float(np.abs(c["e_" + which][k][n]).max())
        rest = max(float(np.abs(np.delete(a, n, axis=0) if a is c["e_" + which][k] else a).max()) for a in arrs)
        out.append(region / rest)
    return out
