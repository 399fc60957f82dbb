"""The translator as a differentiable torch module: forward and backward run in libctxtrans's HIP kernels
(ctx_dev_forward_vjp / ctx_dev_backward_vjp), torch.autograd sees one op.

    mod = TranslatorModule(H=36, W=64, featsize=100, max_batch=32, variant="real", device=0)
    out, out2, input_z, translated_z, loss = mod(src, ctx, tgt)          # cuda f32 [B,H,W,C] frames
    (F.l1_loss(out, tgt) + 0.1 * translated_z.pow(2).sum() + loss).backward()
    opt.step()                                                           # any torch optimiser over mod.parameters()

The parameters live in a torch-owned arena the handle was created on (ctx_create_ex, as dp.RcclTrainer does): `flat` is one
nn.Parameter over its parameter slice, in the handle's layout (ctx_param_info order; ContextAEReal keeps its channel-padded
layout, whose padding entries stay 0 and get gradient 0).  A torch write to `flat` is seen through its `_version` and reported
with ctx_params_written before the next forward.

One live graph per handle: a backward whose forward was followed by another forward (or any other call that runs the
translator) raises RuntimeError, and so does a second backward through the same graph (retain_graph=True).

Not imported by the package's __init__: the package stays importable without torch.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .translator import Translator


class _TranslatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, src, c, tgt, mod):
        ctx.set_materialize_grads(False)                     # unused outputs reach backward as None: a NULL (zero) cotangent
        B = src.shape[0]
        tr = mod.translator
        cur = torch.cuda.current_stream(mod.device)
        mod.stream.wait_stream(cur)
        with torch.cuda.stream(mod.stream):
            token = tr.dev_forward_vjp(src.data_ptr(), c.data_ptr(), tgt.data_ptr(), B, dropout=mod.training, drop_step=mod.drop_step)
            o, o2, iz, tz = (ctypes.c_void_p() for _ in range(4))
            tr._ck(tr._lib.ctx_dev_outputs(tr._h, *(ctypes.byref(p) for p in (o, o2, iz, tz))))
            npi = mod.H * mod.W * mod.C
            out = mod._wrap(o.value, B * npi).view(B, mod.H, mod.W, mod.C).clone()
            out2 = mod._wrap(o2.value, B * npi).view(B, mod.H, mod.W, mod.C).clone()
            iz_t = mod._wrap(iz.value, B * mod.Fp).view(B, mod.Fp)[:, : mod.featsize].clone()
            tz_t = mod._wrap(tz.value, B * mod.Fp).view(B, mod.Fp)[:, : mod.featsize].clone()
            scal = mod._wrap(tr.scalars_ptr, 4).clone()
        cur.wait_stream(mod.stream)
        for t in (out, out2, iz_t, tz_t, scal):
            t.record_stream(cur)
        for t in (src, c, tgt):
            t.record_stream(mod.stream)
        ctx.mod, ctx.token, ctx.B = mod, token, B
        ctx.mark_non_differentiable(scal)
        return out, out2, iz_t, tz_t, scal[0].clone(), scal

    @staticmethod
    def backward(ctx, g_out, g_out2, g_iz, g_tz, g_loss, _g_scal):
        mod, B = ctx.mod, ctx.B
        tr = mod.translator
        dev = mod.device
        cur = torch.cuda.current_stream(dev)

        def ptr(t):
            return None if t is None else t.contiguous().data_ptr()

        keep = [t.contiguous() if t is not None else None for t in (g_out, g_out2, g_iz, g_tz)]
        need = ctx.needs_input_grad
        frames = [torch.empty(B, mod.H, mod.W, mod.C, device=dev, dtype=torch.float32) if need[i] else None for i in (1, 2, 3)]
        lw = float(g_loss.item()) if g_loss is not None else 0.0     # (the ABI takes loss_weight by value: one host read)
        mod.stream.wait_stream(cur)
        with torch.cuda.stream(mod.stream):
            try:
                tr.dev_backward_vjp(ctx.token, *(ptr(t) for t in keep), loss_weight=lw,
                                    d_src_frames=ptr(frames[0]), d_ctx_frames=ptr(frames[1]), d_tgt_frames=ptr(frames[2]))
            except _lib.CtxError as e:
                if e.code == _lib.CTX_E_STATE:
                    raise RuntimeError("TranslatorModule: the forward this backward belongs to was overwritten by a later call on the "
                                       "same handle, or its backward already ran (one live graph per handle; no retain_graph)") from e
                raise
            # a COPY: the next VJP overwrites the gradient arena, while torch may still accumulate this one into .grad
            gflat = mod.grads.clone() if need[0] else None
        cur.wait_stream(mod.stream)
        if gflat is not None:
            gflat.record_stream(cur)
        for t in frames + keep:
            if t is not None:
                t.record_stream(mod.stream)
        return gflat, frames[0], frames[1], frames[2], None


class TranslatorModule(torch.nn.Module):
    def __init__(self, H=64, W=64, df_dim=64, featsize=1024, max_batch=256, device=0, seed=0, **translator_kw):
        """translator_kw: Translator's variant / precision ("f32" | "bf16x3" | "fp16x3" | "fp16x3d") / C / strides / kernels / filters / keep_prob / ablation_type."""
        super().__init__()
        self.device = torch.device("cuda", device)
        kw = {k: translator_kw[k] for k in ("variant", "C", "strides", "kernels", "filters") if k in translator_kw}
        n = Translator.arena_floats(H, W, df_dim, featsize, **kw)
        self._arena = torch.zeros(n, device=self.device, dtype=torch.float32)
        self.stride = n // 4
        torch.cuda.synchronize(self.device)      # the zero-fill ran on torch's stream
        self.stream = torch.cuda.Stream(self.device)
        self.translator = Translator(H, W, df_dim, featsize, max_batch, device=device, stream=self.stream.cuda_stream,
                                     arena_ptr=self._arena.data_ptr(), **translator_kw)
        tr = self.translator
        self.H, self.W, self.C, self.featsize = H, W, tr.C, featsize
        self.Fp = featsize if tr.variant != "real" else -(-featsize // 32) * 32
        self.flat = torch.nn.Parameter(self._arena[: self.stride])       # a view: the handle reads what torch writes
        self.grads = self._arena[self.stride: 2 * self.stride]
        self._index = self._layout()                                     # TF-order element -> arena position
        tr.init_params(seed)
        self.stream.synchronize()
        self.drop_step = 0
        self._seen_version = self.flat._version

    # ---------------------------------------------------------------- layout
    def _layout(self):
        """Arena position of every element of every TF variable (ctx_param_info order), read back from the handle itself: the
        table-driven variants may keep channel-padded tensors in the arena (ContextAEReal does); ContextSkipNew is dense (0 .. P-1)."""
        tr = self.translator
        P = tr.n_params
        if tr.variant == "skipnew":
            return None
        if P >= 1 << 24:
            raise ValueError("TranslatorModule: layout recovery needs fewer than 2^24 parameters")
        idx = np.arange(P, dtype=np.int64)
        pieces = []
        for shift in (0, 12):                               # element index in two 12-bit pieces, each + 1 (exact in f32; padding stays 0)
            tr.set_params_flat(((idx >> shift) & 4095).astype(np.float32) + 1.0)
            self.stream.synchronize()
            pieces.append(self._arena[: self.stride].cpu().numpy().astype(np.int64))
        at = np.nonzero(pieces[0])[0]
        if at.size != P:
            raise RuntimeError("TranslatorModule: could not recover the parameter layout")
        elem = (pieces[0][at] - 1) + ((pieces[1][at] - 1) << 12)
        pos = np.empty(P, np.int64)
        pos[elem] = at
        self._arena[: self.stride].zero_()
        torch.cuda.synchronize(self.device)
        return torch.as_tensor(pos, device=self.device)

    def named_tf(self, t=None):
        """{tf_variable_name: tensor of its TF shape} over `t` (default: the parameters; pass flat.grad for the gradients).  Views for
        dense layouts; gathered copies for ContextAEReal's channel-padded tensors."""
        t = self.flat if t is None else t
        out = {}
        for name, shape, off in self.translator.param_info():
            size = int(np.prod(shape))
            if self._index is None:
                out[name] = t[off: off + size].view(shape)
            else:
                out[name] = t[self._index[off: off + size]].view(shape)
        return out

    def set_params(self, tree):
        """{tf_variable_name: array}, as Translator.set_params (written through the handle, in its layout)."""
        torch.cuda.current_stream(self.device).synchronize()
        self.translator.set_params(tree)
        self.stream.synchronize()
        self._seen_version = self.flat._version

    # ---------------------------------------------------------------- forward
    def _wrap(self, ptr, n):
        holder = type("_DevArr", (), {"__cuda_array_interface__": {"shape": (n,), "typestr": "<f4", "version": 2,
                                                                     "data": (int(ptr), False)}})()
        return torch.as_tensor(holder, device=self.device)

    def forward(self, src, ctx, tgt):
        """src / ctx / tgt: cuda f32 [B,H,W,C].  Returns (out, out2, input_z, translated_z, loss), differentiable; and sets
        self.last_scalars = {simloss, recon1, recon2} (tensors, no gradient)."""
        for t in (src, ctx, tgt):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise ValueError("frames must be cuda float32 tensors")
        src, ctx, tgt = (t.contiguous() for t in (src, ctx, tgt))
        if self.flat._version != self._seen_version:          # a torch optimiser step / copy_ since the last forward
            self.translator.params_written()
            self._seen_version = self.flat._version
        out, out2, iz, tz, loss, scal = _TranslatorFn.apply(self.flat, src, ctx, tgt, self)
        self.last_scalars = dict(simloss=scal[1], recon1=scal[2], recon2=scal[3])
        if self.training:
            self.drop_step += 1
        return out, out2, iz, tz, loss
