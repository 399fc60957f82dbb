"""A float64 statement of an op list of csrc/cnn.cpp (ctx_cnn_*), and the builder the op-level tests make their lists with  --  TEST
INFRASTRUCTURE ONLY.

execute(bufs, ops, blob, frames_u8) restates the five op kinds in plain numpy on oracle.inception_oracle._windows (TF's SAME / VALID
for any kh, kw, stride): conv and linear conv with bias, source slice (src_ch0 / src_c read at the whole buffer's row stride),
destination slice (dst_ch0) and the two-output epilogue (nsplit / dst2 / dst2_ch0); max pool 3x3 stride 2 VALID; average pool 3x3
stride 1 SAME divided by the taps inside the map; avgpool_valid kh x kw stride s.  It returns EVERY buffer at its real (padded)
width; channels no op writes stay zero, as the device's buffers do (allocated zeroed, never written).

tests/test_cnn_ref.py pins the statement itself: on the ops and the folded blob of four Inception layouts it equals
oracle.inception_oracle.forward at every end point to 1e-12.

Case(...) is the compact description -> CnnBuf / CnnOp arrays and a blob with every offset on a multiple of 4; Handle runs it on
the device through ctypes (ctx_cnn_create, ctx_cnn_set_weights, ctx_cnn_forward_u8, ctx_cnn_read_buffer of every buffer)."""
import ctypes
from collections import OrderedDict

import numpy as np

from oracle.ctx_oracle import preprocess_u8
from oracle.inception_oracle import _windows

CONV, MAXPOOL, AVGPOOL, AVGPOOL_VALID, CONV_LINEAR = 0, 1, 2, 3, 4
OP_FIELDS = ("kind", "src", "dst", "dst_ch0", "kh", "kw", "stride", "same", "cout", "lane", "w_off", "b_off", "src_ch0", "src_c", "nsplit",
             "dst2", "dst2_ch0")


def out_grid(h, w, kh, kw, stride, same):
    if same:
        return -(-h // stride), -(-w // stride)
    return (h - kh) // stride + 1, (w - kw) // stride + 1


def execute(bufs, ops, blob, frames_u8, dtype=np.float64):
    """bufs: [(h, w, c)], ops: dicts with OP_FIELDS (missing = 0), blob: the weight blob, frames_u8 [n, H, W, 3] -> one [n, h, w, c]
    array per buffer.  dtype float32 gives the same statement in single precision (the rounding yardstick of the GPU tests)."""
    n = frames_u8.shape[0]
    blob = np.asarray(blob, dtype)
    out = [np.zeros((n,) + tuple(b), dtype) for b in bufs]
    assert frames_u8.shape[1:] == (bufs[0][0], bufs[0][1], 3), (frames_u8.shape, bufs[0])
    out[0][..., :3] = preprocess_u8(frames_u8).astype(dtype)
    for op in ops:
        o = {k: int(op.get(k, 0)) for k in OP_FIELDS}
        x, kind = out[o["src"]], o["kind"]
        if kind in (CONV, CONV_LINEAR):
            cin = o["src_c"] or x.shape[-1]
            x = x[..., o["src_ch0"]:o["src_ch0"] + cin] if o["src_c"] else x
            kh, kw, cout = o["kh"], o["kw"], o["cout"]
            w = blob[o["w_off"]:o["w_off"] + kh * kw * cin * cout].reshape(kh * kw * cin, cout)
            win = _windows(np.ascontiguousarray(x), kh, kw, o["stride"], "SAME" if o["same"] else "VALID")
            N, Ho, Wo = win.shape[:3]
            y = (win.reshape(N * Ho * Wo, -1) @ w).reshape(N, Ho, Wo, cout) + blob[o["b_off"]:o["b_off"] + cout]
            if kind == CONV:
                y = np.maximum(y, 0)
            if o["nsplit"]:
                ns = o["nsplit"]
                out[o["dst"]][..., o["dst_ch0"]:o["dst_ch0"] + ns] = y[..., :ns]
                out[o["dst2"]][..., o["dst2_ch0"]:o["dst2_ch0"] + cout - ns] = y[..., ns:]
            else:
                out[o["dst"]][..., o["dst_ch0"]:o["dst_ch0"] + cout] = y
            continue
        if kind == MAXPOOL:
            y = _windows(x, 3, 3, 2, "VALID").max(axis=(3, 4))
        elif kind == AVGPOOL:
            cnt = _windows(np.ones((1,) + x.shape[1:3] + (1,), dtype), 3, 3, 1, "SAME").sum(axis=(3, 4))
            y = _windows(x, 3, 3, 1, "SAME").sum(axis=(3, 4)) / cnt
        elif kind == AVGPOOL_VALID:
            y = _windows(x, o["kh"], o["kw"], o["stride"], "VALID").sum(axis=(3, 4)) / dtype(o["kh"] * o["kw"])
        else:
            raise ValueError(f"unknown kind {kind}")
        out[o["dst"]][..., o["dst_ch0"]:o["dst_ch0"] + x.shape[-1]] = y
    return out


def written_mask(bufs, ops):
    """Per buffer, a bool [c]: the channels some op writes (buffer 0: the three frame channels)."""
    m = [np.zeros(b[2], bool) for b in bufs]
    m[0][:3] = True
    for op in ops:
        o = {k: int(op.get(k, 0)) for k in OP_FIELDS}
        if o["kind"] in (CONV, CONV_LINEAR):
            n1 = o["nsplit"] or o["cout"]
            m[o["dst"]][o["dst_ch0"]:o["dst_ch0"] + n1] = True
            if o["nsplit"]:
                m[o["dst2"]][o["dst2_ch0"]:o["dst2_ch0"] + o["cout"] - o["nsplit"]] = True
        else:
            m[o["dst"]][o["dst_ch0"]:o["dst_ch0"] + bufs[o["src"]][2]] = True
    return m


def synthetic_tree(convs, seed):
    """InceptionFrontend.init_synthetic's variables for a layout's convs, without a handle."""
    rng = np.random.default_rng(seed)
    tree = OrderedDict()
    for c in convs:
        specs = [(c["scope"] + "/weights", c["k"] + (c["cin"], c["cout"]))]
        if c.get("linear"):
            specs += [(c["scope"] + "/biases", (c["cout"],))]
        else:
            specs += [(c["scope"] + "/BatchNorm/" + n, (c["cout"],)) for n in ("beta", "moving_mean", "moving_variance")]
        for name, shape in specs:
            if name.endswith("weights"):
                tree[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))).astype(np.float32)
            elif name.endswith("moving_variance"):
                tree[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
            else:
                tree[name] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    return tree


# --------------------------------------------------------------------------------------------------------------- the builder
class Case:
    """A small op list.  buf(h, w, c) -> id (c padded to 32); conv(...) / pool(...) append ops and lay their weights into the blob
    (filter [kh][kw][cin][cout] then bias, each conv starting on a multiple of 4; seeded He-scaled filters, biases with spread).
    junk_rows: filter rows [3, cin) of a conv that reads buffer 0 are filled with junk instead of zeros (the frame buffer's padded
    channels are zero, so they must not matter on any route)."""

    def __init__(self, name, H, W, seed=0):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.bufs, self.ops, self.blob, self.seed = [(H, W, 32)], [], [], seed
        self.under_test = None

    def buf(self, h, w, c):
        self.bufs.append((h, w, (c + 31) // 32 * 32))
        return len(self.bufs) - 1

    def _weights(self, kh, kw, cin, cout, real_cin, junk_rows):
        w = self.rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * real_cin))
        if real_cin < cin:
            w[:, :, real_cin:, :] = self.rng.standard_normal((kh, kw, cin - real_cin, cout)) * 7.0 if junk_rows else 0.0
        b = self.rng.standard_normal(cout) * 0.3 + 0.1
        w_off = sum(len(a) for a in self.blob)
        flat = np.concatenate([w.reshape(-1), b]).astype(np.float32)
        flat = np.concatenate([flat, np.zeros(-len(flat) % 4, np.float32)])
        self.blob.append(flat)
        return w_off, w_off + w.size

    def conv(self, src, k, stride, same, cout, dst=None, dst_ch0=0, src_ch0=0, src_c=0, nsplit=0, dst2=None, dst2_ch0=0, linear=False,
             lane=0, junk_rows=False, dst_c=None, real_cin=None):
        kh, kw = k
        h, w, c = self.bufs[src]
        ho, wo = out_grid(h, w, kh, kw, stride, same)
        if dst is None:
            dst = self.buf(ho, wo, dst_c or (nsplit or cout) + dst_ch0)
        if nsplit and dst2 is None:
            dst2 = self.buf(ho, wo, cout - nsplit + dst2_ch0)
        cin = src_c or c
        w_off, b_off = self._weights(kh, kw, cin, cout, real_cin or (3 if src == 0 else cin), junk_rows)
        self.ops.append(dict(kind=CONV_LINEAR if linear else CONV, src=src, dst=dst, dst_ch0=dst_ch0, kh=kh, kw=kw, stride=stride, same=int(same),
                             cout=cout, lane=lane, w_off=w_off, b_off=b_off, src_ch0=src_ch0, src_c=src_c, nsplit=nsplit, dst2=dst2 or 0,
                             dst2_ch0=dst2_ch0))
        return dst

    def pool(self, kind, src, dst=None, dst_ch0=0, k=(3, 3), stride=None, dst_c=None, lane=0):
        h, w, c = self.bufs[src]
        kh, kw = k
        stride = stride or (2 if kind == MAXPOOL else 1)
        ho, wo = out_grid(h, w, kh, kw, stride, kind == AVGPOOL)
        if dst is None:
            dst = self.buf(ho, wo, dst_c or c + dst_ch0)
        self.ops.append(dict(kind=kind, src=src, dst=dst, dst_ch0=dst_ch0, kh=kh, kw=kw, stride=stride, same=int(kind == AVGPOOL), cout=0, lane=lane,
                             w_off=0, b_off=0))
        return dst

    def mark(self):
        """The op appended last is the op under test."""
        self.under_test = len(self.ops) - 1
        return self

    def weights(self):
        return np.concatenate(self.blob)

    def frames(self, n, seed=None):
        H, W, _ = self.bufs[0]
        return np.random.default_rng(1000 + self.seed if seed is None else seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)

    def reference(self, frames_u8, dtype=np.float64):
        return execute(self.bufs, self.ops, self.weights(), frames_u8, dtype)

    def test_output(self, ref):
        """The channels the op under test writes (both outputs of a merged conv, concatenated), from a list of buffers."""
        o = self.ops[self.under_test]
        if o["kind"] in (CONV, CONV_LINEAR):
            n1 = o["nsplit"] or o["cout"]
            parts = [ref[o["dst"]][..., o["dst_ch0"]:o["dst_ch0"] + n1]]
            if o["nsplit"]:
                parts.append(ref[o["dst2"]][..., o["dst2_ch0"]:o["dst2_ch0"] + o["cout"] - o["nsplit"]])
            return np.concatenate(parts, -1)
        return ref[o["dst"]][..., o["dst_ch0"]:o["dst_ch0"] + self.bufs[o["src"]][2]]


PRECISIONS = {"f32": 0, "bf16x3": 1, "fp16x3": 2, "fp16x3d": 3}


class Handle:
    """A ctx_cnn handle on (bufs, ops, blob) through ctypes.  Options reach it through CTX_* in the environment at create."""

    def __init__(self, bufs, ops, blob, max_images, precision="f32"):
        from imitation_from_observation_amd import _lib
        from imitation_from_observation_amd.translator import Translator
        assert PRECISIONS == {k: Translator.PRECISIONS[k] for k in PRECISIONS}
        self._m, self._lib = _lib, _lib.load()
        self.bufs, self.max_images = [tuple(b) for b in bufs], max_images
        cb = (_lib.CnnBuf * len(bufs))(*[_lib.CnnBuf(*b) for b in bufs])
        co = (_lib.CnnOp * len(ops))(*[_lib.CnnOp(*[int(o.get(k, 0)) for k in OP_FIELDS], 0) for o in ops])
        blob = np.ascontiguousarray(blob, np.float32)
        self._h = ctypes.c_void_p()
        rc = self._lib.ctx_cnn_create(cb, len(bufs), co, len(ops), blob.size, max_images, PRECISIONS[precision], 0, ctypes.c_void_p(0),
                                      ctypes.byref(self._h))
        if rc != _lib.CTX_OK:
            msg = self._lib.ctx_cnn_last_error(None)
            self._h = ctypes.c_void_p()
            raise _lib.CtxError(rc, msg.decode() if msg else "")
        self.set_weights(blob)

    def _ck(self, rc):
        if rc != self._m.CTX_OK:
            msg = self._lib.ctx_cnn_last_error(self._h)
            raise self._m.CtxError(rc, msg.decode() if msg else "")

    def set_weights(self, blob):
        blob = np.ascontiguousarray(blob, np.float32)
        self._ck(self._lib.ctx_cnn_set_weights(self._h, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), blob.size))

    def run(self, frames_u8):
        """One pass over n <= max_images frames -> every buffer [n, h, w, c] (f32)."""
        fr = np.ascontiguousarray(frames_u8)
        n = fr.shape[0]
        assert fr.dtype == np.uint8 and n <= self.max_images
        self._ck(self._lib.ctx_cnn_forward_u8(self._h, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, None))
        out = []
        for i, b in enumerate(self.bufs):
            a = np.empty((n,) + b, np.float32)
            self._ck(self._lib.ctx_cnn_read_buffer(self._h, i, n, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
            out.append(a)
        return out

    def close(self):
        if self._h.value:
            self._lib.ctx_cnn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))
