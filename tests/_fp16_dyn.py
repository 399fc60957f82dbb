"""numpy restatement of the fp16x3d operand format (csrc/igemm_split.h, SPLIT_FP16D; csrc/kernels.hip, split_absmax): the three
fp16 terms of tests/_fp16_split.py with one power-of-two scale PER OPERAND,
    e = 14 - (exponent field of the operand's largest |x| - 127), clamped to [-126, 126];  all-zero operand: e = 0
so that the largest entry lands in [2^14, 2^15), and the product rescaled by 2^-e_a and 2^-e_b.  An inf / NaN entry makes the
operand's scale NaN: the whole product is NaN.  Accumulation in float64, rounded to f32 once, as in _fp16_split."""
import numpy as np

from tests._fp16_split import split

E_MIN, E_MAX = -126, 126


def exponent(x):
    """The operand's exponent e, or None where its largest magnitude is not finite."""
    bits = int((np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)).max())      # the kernel's integer maximum
    field = bits >> 23
    if field == 255:
        return None
    if bits == 0:
        return 0
    return int(np.clip(14 - (field - 127), E_MIN, E_MAX))


def matmul3d(a, b):
    """[M, K] x [K, N], each operand split as x * 2^e with its own e; f32 result."""
    ea, eb = exponent(a), exponent(b)
    if ea is None or eb is None:
        return np.full((a.shape[0], b.shape[1]), np.nan, np.float32)
    ah, al = (t.astype(np.float64) for t in split(a, ea))
    bh, bl = (t.astype(np.float64) for t in split(b, eb))
    acc = al @ bh + ah @ bl + ah @ bh
    f1, f2 = sorted((2.0 ** -ea, 2.0 ** -eb))                  # the smaller factor first, as the kernel applies them
    with np.errstate(over="ignore"):
        return ((acc * f1) * f2).astype(np.float32)
