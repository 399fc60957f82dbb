"""numpy restatement of the fp16x3 operand format (csrc/igemm_split.h, SPLIT_FP16): every f32 operand x is split into
    y = x * 2^EXP (f32),  hi = fp16(y),  lo = fp16(y - hi)          (both round-to-nearest-even, fp16 subnormals kept)
and a product is a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, rescaled by 2^(-2 EXP).  The accumulation here is float64, rounded to f32
once at the end: the emulation states the FORMAT's error (what the dropped lo*lo term and fp16's range cost), not the summation
order of the matrix cores."""
import numpy as np

EXP = 6     # CTX_FP16_EXP


def split(x, exp=EXP):
    """f32 array -> (hi, lo) as float16 arrays of x * 2^exp; |x| * 2^exp >= 65520 gives hi = +-inf (and lo = NaN)."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(x, np.float32) * np.float32(2.0 ** exp)
        hi = y.astype(np.float16)
        lo = (y - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def matmul3(a, b, exp=EXP):
    """[M, K] x [K, N] with both operands in the three-term split-fp16 format; f32 result."""
    ah, al = (t.astype(np.float64) for t in split(a, exp))
    bh, bl = (t.astype(np.float64) for t in split(b, exp))
    with np.errstate(over="ignore", invalid="ignore"):
        acc = al @ bh + ah @ bl + ah @ bh                       # small terms first, as the kernel orders them
        return (acc * 2.0 ** (-2 * exp)).astype(np.float32)


def split_bf16(x):
    """The bf16x3 format for comparison: (hi, lo) as f32 arrays holding bf16 values (round-to-nearest-even)."""
    def rne(v):
        u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    x = np.asarray(x, np.float32)
    hi = rne(x)
    return hi, rne(x - hi)


def matmul3_bf16(a, b):
    ah, al = (t.astype(np.float64) for t in split_bf16(a))
    bh, bl = (t.astype(np.float64) for t in split_bf16(b))
    return (al @ bh + ah @ bl + ah @ bh).astype(np.float32)
