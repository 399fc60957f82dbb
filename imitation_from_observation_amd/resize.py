"""`scipy.misc.imresize(img, idims)` on the device: the resize every frame of the reference goes through first (the environments'
render on every step, scripts/train_script.py:16-19 on every demo frame, the third-person trainers).  `FrameResizer` is one plan of
libctxtrans.so's ctx_resize handle (include/ctxtrans.h): raw uint8 frames go up once, Pillow's two fixed-point BILINEAR passes run
as HIP kernels, and the result comes back as uint8 -- equal to `demo_pipeline.imresize_bilinear_u8` and to Pillow bit for bit -- or
stays on the device: as f32 in the sampler's (x/255 - 0.5)*2 form, which is what the `_dev` entries of `Translator` /
`InceptionFrontend` take, or as the same uint8 bytes, which is what the Inception-feature reward and the discriminators take.
ctypes only."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import CtxError

_UP = ctypes.POINTER(ctypes.c_uint8)
_IP = ctypes.POINTER(ctypes.c_int32)


class FrameResizer:
    def __init__(self, in_size, out_size, max_frames=250, device=0, stream=None):
        """in_size (Hin, Win) -> out_size (Hout, Wout), frames uint8 [.., 3]; max_frames: the most frames one device pass holds
        (`resize` chunks longer inputs, `resize_dev` refuses them).  stream: integer hipStream_t of the consumer
        (Translator.stream_ptr(), InceptionFrontend.stream) so that its `_dev` entries read the result in stream order; None = a
        private stream (`sync()` before another stream reads)."""
        self._lib = _lib.load()
        self.in_size, self.out_size = (int(in_size[0]), int(in_size[1])), (int(out_size[0]), int(out_size[1]))
        self.max_frames, self.device = int(max_frames), int(device)
        self._h = ctypes.c_void_p()
        self._pending, self._pending_own = None, False
        rc = self._lib.ctx_resize_create(self.in_size[0], self.in_size[1], 3, self.out_size[0], self.out_size[1], self.max_frames,
                                         self.device, ctypes.c_void_p(stream or 0), ctypes.byref(self._h))
        if rc != _lib.CTX_OK:
            msg = self._lib.ctx_resize_last_error(None)
            self._h = ctypes.c_void_p()
            raise CtxError(rc, msg.decode() if msg else "")

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ctx_resize_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._pending, self._pending_own = None, False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, rc):
        if rc != _lib.CTX_OK:
            msg = self._lib.ctx_resize_last_error(self._h)
            raise CtxError(rc, msg.decode() if msg else "")

    # ------------------------------------------------------------------ tables (no device)
    @staticmethod
    def coeffs(in_size, out_size):
        """(xmin [out], count [out], kk [out, ksize]) int32 of one axis: Pillow's precompute_coeffs + normalize_coeffs_8bpc as the
        library computes them on the host (= demo_pipeline._coeffs).  Needs no device."""
        lib = _lib.load()
        ks = ctypes.c_int()
        rc = lib.ctx_resize_coeffs(int(in_size), int(out_size), None, None, None, ctypes.byref(ks))
        if rc != _lib.CTX_OK:
            msg = lib.ctx_resize_last_error(None)
            raise CtxError(rc, msg.decode() if msg else "")
        xmin, cnt = np.empty(int(out_size), np.int32), np.empty(int(out_size), np.int32)
        kk = np.empty((int(out_size), ks.value), np.int32)
        rc = lib.ctx_resize_coeffs(int(in_size), int(out_size), xmin.ctypes.data_as(_IP), cnt.ctypes.data_as(_IP), kk.ctypes.data_as(_IP),
                                   ctypes.byref(ks))
        if rc != _lib.CTX_OK:
            msg = lib.ctx_resize_last_error(None)
            raise CtxError(rc, msg.decode() if msg else "")
        return xmin, cnt, kk

    # ------------------------------------------------------------------ the two fetches
    def _frames(self, frames_u8):
        fr = np.asarray(frames_u8)
        if fr.dtype != np.uint8:
            raise TypeError(f"expected uint8 frames, got {fr.dtype}")
        single = fr.ndim == 3
        if single:
            fr = fr[None]
        if fr.ndim != 4 or fr.shape[1:] != self.in_size + (3,) or fr.shape[0] < 1:
            raise ValueError(f"frames must be uint8 [n,{self.in_size[0]},{self.in_size[1]},3] (or one frame), got {fr.shape}")
        return np.ascontiguousarray(fr), single

    def resize(self, frames_u8):
        """uint8 [n, Hin, Win, 3] (any n >= 1) -> uint8 [n, Hout, Wout, 3]; one frame [Hin, Win, 3] -> one frame.  Synchronous."""
        fr, single = self._frames(frames_u8)
        out = np.empty((fr.shape[0],) + self.out_size + (3,), np.uint8)
        self._ck(self._lib.ctx_resize_u8(self._h, fr.ctypes.data_as(_UP), fr.shape[0], out.ctypes.data_as(_UP)))
        return out[0] if single else out

    def _frame_list(self, frames):
        """A list of n uint8 [Hin, Win, 3] frames -> (kept arrays, ctypes array of their addresses, whether a copy was made here).
        Contiguous entries are uploaded from where they are; a non-contiguous one is copied first."""
        keep, own = [], False
        for f in frames:
            a = np.asarray(f)
            if a.dtype != np.uint8:
                raise TypeError(f"expected uint8 frames, got {a.dtype}")
            if a.shape != self.in_size + (3,):
                raise ValueError(f"every frame must be uint8 [{self.in_size[0]},{self.in_size[1]},3], got {a.shape}")
            keep.append(a if a.flags.c_contiguous else np.ascontiguousarray(a))
            own = own or keep[-1] is not f
        if not keep:
            raise ValueError("no frames")
        ptrs = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
        return keep, ptrs, own

    def _hold(self, keep, own):
        """The frames the queued uploads read.  A copy made here has no owner but this object, so the uploads of the call before are
        waited for before such a copy is let go; frames the caller owns are the caller's to keep until the next call / sync."""
        if self._pending_own:
            self.sync()
        self._pending, self._pending_own = keep, own

    def _dev(self, block_fn, list_fn, frames_u8, dst):
        d_out = ctypes.c_void_p()
        if isinstance(frames_u8, (list, tuple)):
            keep, ptrs, own = self._frame_list(frames_u8)
            self._hold((keep, ptrs), own)                         # the uploads read the frames in stream order
            self._ck(list_fn(self._h, ptrs, len(keep), ctypes.c_void_p(dst or 0), ctypes.byref(d_out)))
        else:
            fr, _ = self._frames(frames_u8)
            # `fr` is the caller's memory only if the caller passed an ndarray that was already contiguous; anything else (a nested
            # list, a strided view) was copied by _frames, and that copy is this object's
            caller_owns = isinstance(frames_u8, np.ndarray) and np.may_share_memory(fr, frames_u8)
            self._hold(fr, not caller_owns)
            self._ck(block_fn(self._h, fr.ctypes.data_as(_UP), fr.shape[0], ctypes.c_void_p(dst or 0), ctypes.byref(d_out)))
        return int(d_out.value)

    def resize_dev(self, frames_u8, dst=None):
        """uint8 [n, Hin, Win, 3] (n <= max_frames), or a list of n uint8 [Hin, Win, 3] frames (uploaded one by one from where they
        are, no gather on the host) -> integer DEVICE address of f32 [n, Hout, Wout, 3] in (x/255 - 0.5)*2 form.
        dst: integer device address to write to (n*Hout*Wout*3 floats, e.g. Translator.dev_frames(n)[0]); None = the plan's own
        buffer, valid until the next call.  Asynchronous on the plan's stream; the frames are kept alive by this object until
        the next call / sync."""
        return self._dev(self._lib.ctx_resize_f32_dev, self._lib.ctx_resize_f32_dev_v, frames_u8, dst)

    def resize_u8_dev(self, frames_u8, dst=None):
        """The same input forms as resize_dev -> integer DEVICE address of uint8 [n, Hout, Wout, 3], the bytes `resize` returns: what
        InceptionFrontend.features_from_dev_u8 / reward_costs_dev_u8 and the discriminators' reward_paths_dev take.  dst: any device
        byte address with n*Hout*Wout*3 bytes behind it (e.g. an offset into the tensor of data_begin); None = the plan's own uint8
        buffer, valid until the next call (the input buffer itself when the sizes are equal)."""
        return self._dev(self._lib.ctx_resize_u8_dev, self._lib.ctx_resize_u8_dev_v, frames_u8, dst)

    def sync(self):
        self._ck(self._lib.ctx_resize_sync(self._h))
        self._pending, self._pending_own = None, False

    def profile(self, frames_u8, pinned=False):
        """Measurement only (tools/bench_resize.py): (h2d_ms, kernel_ms) of one upload of the frames and one run of the kernels,
        between HIP events on the plan's stream."""
        fr, _ = self._frames(frames_u8)
        a, b = ctypes.c_float(), ctypes.c_float()
        self._ck(self._lib.ctx_resize_profile(self._h, fr.ctypes.data_as(_UP), fr.shape[0], int(bool(pinned)), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value
