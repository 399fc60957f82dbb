"""mode == 'oursinception' of the reward hook (rllab/sampler/base.py:121-132): frames -> frozen Inception-v3 ->
Mixed_7c feature maps -> ContextAEInception2.  `InceptionTranslator` chains the two device handles behind the same
translate / encode surface as `Translator`, so `TranslatorReward` runs unchanged; in this mode the 'image' the cost
compares is the feature tensor (base.py:132: self.image_trans = featreshape).

Both handles share ONE stream and the feature maps stay in HBM: frames go up as uint8, the front end writes Mixed_7c into its
output buffer, the translator reads that buffer through device pointers (ctx_cnn_forward_u8_dev -> ctx_translate_dev /
ctx_encode_dev / ctx_dev_forward_backward), and only codes, predicted feature maps and scalars come back.

The trainer's surface (scripts/train_script.py:144-203, trainer.ModelTrainer): the host-fed steps train_step_u8 / evaluate_u8, and --
with the demo tensor resident in the front end (load_demos) -- the sampled steps on one GPU (train_step_sampled / eval_sampled) and
data parallel (dp_*): every rank holds the whole uint8 tensor, gathers its rows of the GLOBAL batch on the device and runs the front
end on them per step, as the reference graph does; the translator's step is the bucketed RCCL step of ctx_dp_train_step on the maps.
nn_err / dp_nn_err compare output maps with tgt maps where they are."""
from __future__ import annotations

import numpy as np

from .inception_frontend import InceptionFrontend
from .translator import Translator


class InceptionTranslator:
    def __init__(self, imsize=(125, 125), max_batch=25, device=0, precision=None, df_dim=64, featsize=1024, stream=None,
                 strides=None, kernels=None, filters=None, train=True):
        """precision: "f32" | "bf16x3" | "fp16x3" | "fp16x3d" for BOTH handles (Translator.__init__); None = f32 front end, the translator's default."""
        # the front end sees src + ctx (+ tgt when training) frames of one batch in a single pass: 3 * max_batch images for the
        # trainer, 2 * max_batch for the reward hook (train=False: translate = B + B, encode = B), which sizes every activation buffer
        self.train = bool(train)
        self.front = InceptionFrontend(imsize[0], imsize[1], max_images=(3 if train else 2) * max_batch, device=device,
                                       precision=precision or "f32", stream=stream)
        h, w, c = self.front.out_shape
        self.tr = Translator(h, w, df_dim, featsize, max_batch=max_batch, device=device, variant="inception2", C=c,
                             precision=precision, stream=self.front.stream, strides=strides, kernels=kernels, filters=filters)
        self.H, self.W, self.featsize, self.max_batch = imsize[0], imsize[1], featsize, max_batch
        self.pred_shape = (h, w, c)
        self._per = h * w * c * 4                          # bytes of one image's feature maps

    def close(self):
        self.tr.close()
        self.front.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def translate(self, obs_src, obs_tgt0):
        """uint8 frames [B,H,W,3] and the context frame [H,W,3] (or [B,H,W,3]) -> (translated feature maps, translated_z):
        sess.run([model.translated_z, model.out], {image: [src, [ctx]*B, [ctx]*B]}), base.py:216-218."""
        src = np.asarray(obs_src)
        ctx = np.asarray(obs_tgt0)
        batched = ctx.ndim == 4
        B = src.shape[0]
        d = self.front.features_u8_dev(np.concatenate([src, ctx if batched else ctx[None]]))
        return self.tr.translate_dev(d, d + B * self._per, B, ctx_batched=batched)

    def encode(self, frames, return_frames=True):
        """(input_z, image_trans[0]) of base.py:234-235 -- image_trans is the feature tensor in this mode (the reward's image term
        compares feature maps, so they do come back to the host here: 32 KB per 125x125 frame)."""
        fr = np.asarray(frames)
        d = self.front.features_u8_dev(fr)
        feat = self.tr.encode_dev(d, fr.shape[0])
        return feat, (self.front.output(fr.shape[0]) if return_frames else None)

    # ------------------------------------------------------------------ the reward hook with maps and demo cache resident on the device
    # (TranslatorReward(resident=True)).  Deliberately NOT named reward_set_cache / reward_costs: those names are what the host-path
    # hook (resident=False) dispatches on, and with it this class keeps today's path bit for bit.
    def reward_costs_u8(self, vp, frames, scale, ablation_type="None"):
        """uint8 frames [npaths*bs,H,W,3] -> costs f32 [npaths, bs] of base.py:243-249: frames -> front end -> the translator's
        encoder and cost kernel on the front end's output buffer (the image term compares feature maps, base.py:132).  Only the
        costs come back."""
        fr = np.asarray(frames)
        bs = self.tr._reward_bs
        if fr.shape[0] % bs:
            raise ValueError(f"frames must be [npaths*{bs},H,W,3], got {fr.shape}")
        d = self.front.features_u8_dev(fr)
        return self.tr.reward_costs_dev(vp, d, fr.shape[0] // bs, scale, ablation_type)

    def reconstruct(self, frames, ctx0=None, nctx=1):
        """(out2, input_z) of the feed [frames, ctx, frames] on uint8 frames [B,H,W,3] (Translator.reconstruct): frames (and explicit
        contexts [nctx,H,W,3]) through the front end in one pass, the translator on its output buffer; out2 is a feature map here."""
        fr = np.asarray(frames)
        B = fr.shape[0]
        if ctx0 is None:
            return self.tr.reconstruct_dev(self.front.features_u8_dev(fr), B, None, nctx)
        d = self.front.features_u8_dev(np.concatenate([fr, np.asarray(ctx0)]))
        return self.tr.reconstruct_dev(d, B, d + B * self._per, nctx)

    def reward_costs_recon_u8(self, vp, frames, scale):
        """uint8 frames [npaths*bs,H,W,3] -> costs f32 [npaths, bs] of the 'recon' ablation (Translator.reward_costs_recon): front end,
        then encoder, decoder pass 2 and the row-wise cost on its output buffer.  Only the costs come back."""
        fr = np.asarray(frames)
        bs = self.tr._reward_bs
        if fr.shape[0] % bs:
            raise ValueError(f"frames must be [npaths*{bs},H,W,3], got {fr.shape}")
        return self.tr.reward_costs_recon_dev(vp, self.front.features_u8_dev(fr), fr.shape[0] // bs, scale)

    def reward_cache_begin(self, vp, bs):
        self.tr.reward_cache_begin(vp, bs)

    def reward_cache_add(self, vp, obs_src, obs_tgt0):
        """uint8 demo frames [nvideos*bs,H,W,3] and the ONE context frame [H,W,3]: [src | ctx] through the front end in one pass (as
        translate), then the translator adds translated_z / out of every video to the device sums."""
        src = np.asarray(obs_src)
        ctx = np.asarray(obs_tgt0)
        bs = getattr(self.tr, "_cache_bs", 0)
        if not bs or ctx.ndim != 3 or src.shape[0] % bs:
            raise ValueError(f"expected [nvideos*{bs},H,W,3] frames and one [H,W,3] context after reward_cache_begin")
        B = src.shape[0]
        d = self.front.features_u8_dev(np.concatenate([src, ctx[None]]))
        self.tr.reward_cache_add_dev(vp, d, d + B * self._per, B // bs)

    def reward_cache_finish(self, vp, nvideos_total, distributed=False):
        self.tr.reward_cache_finish(vp, nvideos_total, distributed)

    def reward_get_cache(self, vp, means=True, imgs=True):
        return self.tr.reward_get_cache(vp, means, imgs)

    def reward_stats(self):
        return self.tr.reward_stats()

    def _triple_dev(self, src, ctx, tgt):
        B = len(src)
        if 3 * B > self.front.max_images:
            raise ValueError(f"{B} triples need {3 * B} front-end images, the handle holds {self.front.max_images}"
                             + ("" if self.train else " (built with train=False: the reward hook's two fetches only)"))
        d = self.front.features_u8_dev(np.concatenate([src, ctx, tgt]))
        return d, d + B * self._per, d + 2 * B * self._per, B

    def train_step_u8(self, src, ctx, tgt, lr=1e-4):
        """One Adam step of the translator on uint8 frame triples (scripts/train_script.py:98-114, 163); the front end is frozen."""
        ds, dc, dt, B = self._triple_dev(src, ctx, tgt)
        self.tr.dev_forward_backward(ds, dc, dt, B)
        self.tr.dev_adam(lr)
        return self.tr.dev_scalars()

    def evaluate_u8(self, src, ctx, tgt, outputs=True):
        """The trainer's validation fetch (train_script.py:176) on uint8 frames: loss, simloss, recon1, recon2 (+ out, out2 and the
        tgt feature maps the nn_err fetch compares with, :148)."""
        ds, dc, dt, B = self._triple_dev(src, ctx, tgt)
        self.tr.dev_forward(ds, dc, dt, B)
        res = self.tr.dev_scalars()
        if outputs:
            res["out"], res["out2"], res["tgt"] = self.tr.last_outputs(out=True, out2=True, tgt=True)
        return res

    # ------------------------------------------------------------------ the trainer's sampled steps (resident demo tensor)
    def load_demos(self, vdata_u8):
        """Keep the trainer's demo tensor vdata[T,N,H,W,3] (uint8 frames) resident in the front end (ctx_cnn_demos_upload)."""
        self.front.load_demos(vdata_u8)
        self.demo_shape = self.front.demo_shape

    def _sampled_dev(self, choicesrc, choicetgt, rank=0, world=1):
        cs = np.ascontiguousarray(choicesrc, dtype=np.int32)
        ct = np.ascontiguousarray(choicetgt, dtype=np.int32)
        if cs.shape != ct.shape or cs.ndim != 1:
            raise ValueError("choicesrc / choicetgt must be 1-D and equally long")
        B = cs.size // world
        d = self.front.features_sampled_dev(cs, ct, cs.size, rank, world)
        return d, d + B * self._per, d + 2 * B * self._per, B

    def train_step_sampled(self, choicesrc, choicetgt, lr=1e-4):
        """train_step_u8 on the batch the trainer samples (train_script.py:153-163), gathered from the resident tensor on the device:
        the same calls on the same maps, so the same bits."""
        ds, dc, dt, B = self._sampled_dev(choicesrc, choicetgt)
        self.tr.dev_forward_backward(ds, dc, dt, B)
        self.tr.dev_adam(lr)
        return self.tr.dev_scalars()

    def eval_sampled(self, choicesrc, choicetgt, outputs=True):
        """evaluate_u8 on the sampled validation batch (train_script.py:169-176)."""
        ds, dc, dt, B = self._sampled_dev(choicesrc, choicetgt)
        self.tr.dev_forward(ds, dc, dt, B)
        res = self.tr.dev_scalars()
        if outputs:
            res["out"], res["out2"], res["tgt"] = self.tr.last_outputs(out=True, out2=True, tgt=True)
        return res

    def nn_err(self, nlen, j0=0):
        """trainer.nn_err of the last training-mode forward on the device: output maps against the tgt maps it was fed."""
        return self.tr.nn_err(nlen, j0)

    def last_outputs(self, out=True, out2=False, tgt=False):
        return self.tr.last_outputs(out=out, out2=out2, tgt=tgt)

    def save(self, path, with_adam=True, prefix="", weights="params"):
        return self.tr.save(path, with_adam=with_adam, prefix=prefix, weights=weights)

    def load(self, path, prefix=""):
        self.tr.load(path, prefix=prefix)

    # ------------------------------------------------------------------ data parallel (one process per GPU)
    @staticmethod
    def dp_unique_id():
        return Translator.dp_unique_id()

    def dp_init(self, unique_id, rank, world):
        """Collective: the translator joins the RCCL group (rank 0's parameters and Adam slots reach every replica); the front end is
        frozen and needs no exchange."""
        self.tr.dp_init(unique_id, rank, world)

    def dp_world(self):
        return self.tr.dp_world()

    def dp_allreduce_host(self, arr):
        return self.tr.dp_allreduce_host(arr)

    def dp_scalars(self):
        return self.tr.dp_scalars()

    def _rank_world(self):
        rank, world = self.tr.dp_world()
        if world < 1:
            raise ValueError("dp_init first")
        return rank, world

    def dp_train_step_sampled(self, choicesrc, choicetgt, lr=1e-4, scalars=True):
        """One data-parallel step: this rank's rows of the GLOBAL batch through the front end (on the device, from the resident tensor),
        then ctx_dp_train_step on the maps (simloss mean over the global batch, bucketed gradient all-reduce, Adam).  Returns the
        GLOBAL dict(loss, simloss, recon1, recon2) when scalars."""
        rank, world = self._rank_world()
        ds, dc, dt, B = self._sampled_dev(choicesrc, choicetgt, rank, world)
        return self.tr.dp_train_step(ds, dc, dt, B, lr=lr, scalars=scalars)

    def dp_eval_sampled(self, choicesrc, choicetgt, outputs=True):
        """The validation fetch sharded over the ranks (collective): GLOBAL scalars and -- outputs=True -- out / out2 / tgt maps of THIS
        rank's rows."""
        rank, world = self._rank_world()
        ds, dc, dt, B = self._sampled_dev(choicesrc, choicetgt, rank, world)
        self.tr.dev_forward(ds, dc, dt, B)
        res = self.tr.dp_scalars()
        if outputs:
            res["out"], res["out2"], res["tgt"] = self.tr.last_outputs(out=True, out2=True, tgt=True)
        return res

    def dp_nn_err(self, nlen):
        """nn_err of the GLOBAL batch (collective; ctx_dp_nn_err): the same integer on every rank."""
        return self.tr.dp_nn_err(nlen)
