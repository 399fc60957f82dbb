"""The image-feature reward of the reference's TRPO loop, on top of `Translator`.

Restates the `mode == 'ours'` branch of BaseSampler.process_samples (rllab/sampler/base.py:192-257):
  * once per experiment: translate every demo video into the current context (first rollout frame of
    each viewpoint) and cache the mean translated feature track and mean translated frames
    (base.py:195-223);
  * per path: encode the 25 rollout frames, cost_j = ||means_j - feat_j||^2 + scale * ||imgs_j - x_j||^2
    summed over viewpoints (base.py:232-245), and  rewards[2j+1] -= cost_j * j^2  (base.py:256-257).
The arithmetic on the frames runs in the HIP translator; several paths are encoded per launch (the
encoder is per-frame independent, so results do not depend on the grouping).  The reference's internal
inconsistencies on this path (SURVEY.md 3.4 e-g) are resolved to the intended behaviour and noted inline.

`InceptionFeatureReward` (end of file) is the comparison reward of modes 'inception' / 'inceptionsame' (base.py:69-111, 178-189).
"""
from __future__ import annotations

import numpy as np

from .render_frames import RenderFrames, gather


def apply_costs(paths, costs, batch_size):
    """In place: path['rewards'][2j+1] -= costs[p][j] * j**2 (base.py:256-257; :188-189 in the Inception modes)."""
    for p, c in zip(paths, costs):
        for j in range(batch_size):
            p["rewards"][j * 2 + 1] -= c[j] * (j ** 2)


class _ResidentCacheView:
    """TranslatorReward.means / .imgs of a resident hook: view[vp] fetches that viewpoint's cache from the device (reward_get_cache)."""

    def __init__(self, tr, nvp, which):
        self._tr, self._nvp, self._which = tr, nvp, which

    def __len__(self):
        return self._nvp

    def __getitem__(self, vp):
        if not 0 <= vp < self._nvp:
            raise IndexError(vp)
        return self._tr.reward_get_cache(vp, means=self._which == 0, imgs=self._which == 1)[self._which]

    def __iter__(self):
        return (self[vp] for vp in range(self._nvp))


class TranslatorReward:
    def __init__(self, translator, nvp, scale, name="strike", ablation_type="None", batch_size=25, resident=False, render_size=None,
                 image_recon=None):
        """resident=True: demo cache and cost stay on the device for EVERY translator type (mode 'oursinception' included) -- the cache
        is built there (reward_cache_begin / _add / _finish: neither the translated videos nor the finished cache cross PCIe), the
        per-path cost is computed next to the encoder (reward_costs_u8: only [paths, bs] floats come back), and `means` / `imgs` are
        views that fetch a viewpoint's cache on demand.  resident=False (default): today's paths, bit for bit.
        render_size=(Hr, Wr): env_infos['imgs'] holds the frames as RENDERED, uint8 [Hr, Wr, 3], and the hook resizes them to the
        translator's size itself (scipy.misc.imresize of the environments, on the device: resize.FrameResizer on the translator's
        stream).  Per launch group the raw frames go up once, are resized into f32 where the encoder reads them and go through the
        device cost entry; only the [paths, bs] costs come back.  The costs equal, bit for bit, those of a hook without render_size
        fed the same frames resized on the host.  None (default): frames arrive at the translator's size, as before.
        ablation_type="recon" with image_recon="out2": cost_j = sum((means[vp][j] - input_z[j])^2) + scale * sum((out2[j] -
        image_trans[0][j])^2), out2 = the path's frames reconstructed in the context of the path's first frame (Translator.reconstruct);
        the reconstruction error replaces the distance to the translated demo frames.  Overwrites per viewpoint like the other
        ablations; the feature term still needs the demo cache."""
        if image_recon is not None and ablation_type != "recon":
            raise ValueError("image_recon names the tensor of ablation_type='recon' only")
        if ablation_type == "recon" and image_recon is not None:
            # the launchers' ours_recon (run_trpo_strike.py:87, run_trpo_throw.py:77).  base.py:250-252 reads `image_recon`, which is never
            # assigned; the trainer's __<k>recon.gif = test.out2 (train_script.py:193-195) and the commented base.py:238-241 (image_recon[j]
            # saved next to image_trans[0][j] of the same sess.run) say it was model.out2 of the per-path feed.  The caller names it.
            if image_recon != "out2":
                raise ValueError(f"image_recon={image_recon!r}: 'out2' (model.out2 of the per-path feed) is the only tensor offered")
        elif ablation_type not in ("None", "nofeat", "noimage"):
            # 'recon' reads an undefined `image_recon` in the reference (base.py:250-252): image_recon="out2" names it
            raise NotImplementedError(f"ablation_type {ablation_type!r} is not runnable in the reference either")
        self.image_recon = image_recon
        self.tr, self.nvp, self.scale, self.name = translator, int(nvp), float(scale), name
        self.ablation_type, self.batch_size = ablation_type, int(batch_size)
        self.skip = 2 if name in ("real", "sweep") else 1        # base.py:209-211
        self.resident = bool(resident)
        self._means, self._imgs, self._resident_built = None, None, False
        self.validdata = None                                    # set_demos(): the cache is then built lazily on the first path
        # mode 'oursinception' caps the demo videos at 50 (base.py:203-204); every other mode uses them all
        self.nvideos_cap = 50 if hasattr(translator, "front") else None
        self._render = RenderFrames(render_size, self._resize_plan)
        self.render_size = self._render.size

    _rs = property(lambda self: self._render.rs)                 # the resizer in use (a FrameResizer, made at the first use)

    # means[vp] [bs, featsize] / imgs[vp] [bs, H, W, C]: host lists (resident=False), device-backed views (resident=True); None = no cache yet
    @property
    def means(self):
        if self.resident:
            return _ResidentCacheView(self.tr, self.nvp, 0) if self._resident_built else None
        return self._means

    @means.setter
    def means(self, v):
        self._means = v

    @property
    def imgs(self):
        if self.resident:
            return _ResidentCacheView(self.tr, self.nvp, 1) if self._resident_built else None
        return self._imgs

    @imgs.setter
    def imgs(self, v):
        self._imgs = v

    @classmethod
    def for_sampler(cls, name, imsize, nvp, scale, modelname=None, ablation_type="None", batch_size=25,
                    paths_per_launch=10, device=0, mode="ours", inception_ckpt=None, resident=False, render_size=None, precision=None,
                    image_recon=None):
        """What BaseSampler.initialize() sets up for mode 'ours' (base.py:113-145): the model class follows the
        experiment name -- ContextAEReal for 'real'/'sweep', ContextSkipNew otherwise (:134-137) -- on the
        sampler's imsize, restored from `modelname` when given (:138).  mode 'oursinception' (:121-132): frames go
        through the frozen Inception-v3 (variables from `inception_ckpt`, an .npz keyed by the TF names) and
        ContextAEInception2 runs on the Mixed_7c feature maps.  precision: "f32" | "bf16x3" | "fp16x3" | "fp16x3d" for the Translator /
        InceptionTranslator built here (Translator.__init__ states each mode's error and range); None = their default."""
        from .translator import Translator
        if mode == "oursinception":
            from .oursinception import InceptionTranslator
            it = InceptionTranslator(imsize, max_batch=batch_size * paths_per_launch, device=device, train=False, precision=precision)
            if inception_ckpt is not None:
                it.front.load(inception_ckpt)
            if modelname is not None:
                it.tr.load(modelname)
            return cls(it, nvp, scale, name=name, ablation_type=ablation_type, batch_size=batch_size, resident=resident,
                       render_size=render_size, image_recon=image_recon)
        real = name in ("real", "sweep")
        tr = Translator(imsize[0], imsize[1], featsize=100 if real else 1024, max_batch=batch_size * paths_per_launch,
                        device=device, variant="real" if real else "skipnew", precision=precision)
        if modelname is not None:
            tr.load(modelname)
        return cls(tr, nvp, scale, name=name, ablation_type=ablation_type, batch_size=batch_size, resident=resident, render_size=render_size,
                   image_recon=image_recon)

    # ------------------------------------------------------------------ base.py:195-223
    @staticmethod
    def _frames_of(path):
        """env_infos['imgs'] holds, every other step, a list over viewpoints of uint8 frames (base.py:193)."""
        return [img for img in path["env_infos"]["imgs"] if img is not None]

    def _resize_plan(self):
        """render_size -> the translator's frame size, on the stream the translator's device entries run on (the front end's in mode
        'oursinception'); a translator without a device stream (a host stand-in) gets a private one and the host-array form."""
        front = getattr(self.tr, "front", None)
        stream = front.stream if front is not None else getattr(self.tr, "stream_ptr", None)
        return (self.tr.H, self.tr.W), max(self.tr.max_batch, self.batch_size), getattr(self.tr, "device", getattr(front, "device", 0)), stream

    def _context_frames(self, first_frames):
        """The context frame of every viewpoint (base.py:200) at the translator's size: rendered-size ones are resized to host uint8."""
        if self.render_size is None:
            return first_frames
        out = []
        for f in first_frames:
            f = np.ascontiguousarray(f, dtype=np.uint8)
            out.append(self._render.resizer().resize(f) if f.shape[:2] == self.render_size else f)
        return out

    def set_demos(self, validdata):
        """np.load(self.algo._kwargs['modeldata']) (base.py:198), kept for the lazy cache build of process_paths."""
        self.validdata = np.asarray(validdata)
        return self

    def build_demo_cache(self, validdata, first_frames, distributed=False):
        """validdata: demo tensor [T, Nvid, H, W, 3] in [-1,1] (np.load(modeldata), base.py:198);
        first_frames[vp]: uint8 context frame = first frame of the current rollout (base.py:200).
        In mode 'oursinception' only the first 50 videos are used (`nvideos = 50`, base.py:203-204) and the reference feeds
        `validdata[::skip, i]` to its uint8 placeholder WITHOUT the (x+1)*127.5 conversion (:212-213) -- so a uint8 demo
        tensor is taken as it is there; a float one is converted like in the other modes (deviations).
        distributed=True (one rank per GPU): the demo videos are sharded rank::world, every rank translates its shard and
        the partial feature / frame sums are combined with ONE all-reduce per viewpoint -- the demo means are a plain sum
        over videos.  The group is the translator's own RCCL group when it has one (Translator.dp_init:
        ctx_dp_allreduce_host_f64, no torch in the sampler process), else an initialised torch.distributed group."""
        first_frames = self._context_frames(first_frames)
        if self.resident:
            return self._build_demo_cache_resident(validdata, first_frames, distributed)
        validdata = np.asarray(validdata)
        nvid, bs = self._nvideos(validdata), self.batch_size
        self.means, self.imgs = [], []
        rank, world, allsum = self._group(distributed)
        for vp in range(self.nvp):
            ctx = np.ascontiguousarray(first_frames[vp], dtype=np.uint8)
            fsum = np.zeros((bs, self.tr.featsize), np.float64)
            pshape = tuple(getattr(self.tr, "pred_shape", (self.tr.H, self.tr.W, 3)))   # feature maps in mode 'oursinception'
            isum = np.zeros((bs,) + pshape, np.float64)
            for n, u8 in self._demo_batches(validdata, rank, world):
                timg, tfeat = self.tr.translate(u8, ctx)                   # [translated_z, out], base.py:216-218
                fsum += tfeat.reshape(n, bs, -1).sum(0)
                isum += timg.reshape((n, bs) + pshape).sum(0)
            if world > 1:
                flat = allsum(np.concatenate([fsum.ravel(), isum.ravel()]))
                fsum, isum = flat[:fsum.size].reshape(fsum.shape), flat[fsum.size:].reshape(isum.shape)
            self.means.append((fsum / nvid).astype(np.float32))            # np.mean(tfeats, axis=0), base.py:221
            self.imgs.append((isum / nvid).astype(np.float32))             # np.mean(timgs, axis=0), base.py:222
            if hasattr(self.tr, "reward_set_cache"):                       # the cost is then computed on the device, next to the encoder
                self.tr.reward_set_cache(vp, self.means[vp], self.imgs[vp])
        return self

    def _nvideos(self, validdata):
        return validdata.shape[1] if self.nvideos_cap is None else min(validdata.shape[1], self.nvideos_cap)

    def _demo_batches(self, validdata, rank, world):
        """(videos in the batch, their uint8 frames [videos * bs, H, W, 3]) for the demo videos rank::world below the cap, as many
        whole videos per batch as one translate launch holds."""
        raw_u8 = validdata.dtype == np.uint8
        bs = self.batch_size
        per_call = max(1, self.tr.max_batch // bs)
        mine = list(range(rank, self._nvideos(validdata), world))
        for i0 in range(0, len(mine), per_call):
            vids = mine[i0:i0 + per_call]
            # ((validdata[::skip, i] + 1) * 127.5).astype(np.uint8), base.py:215
            yield len(vids), np.concatenate([validdata[::self.skip, i][:bs] if raw_u8 else
                                             ((validdata[::self.skip, i][:bs] + 1) * 127.5).astype(np.uint8) for i in vids])

    def _build_demo_cache_resident(self, validdata, first_frames, distributed):
        """build_demo_cache with sums and cache on the device: the same videos in the same order through the same translate launches,
        added in float64 and divided once (what the host path does with numpy), but nothing is downloaded and nothing uploaded.
        distributed=True needs the translator's own RCCL group (dp_init): the sums are all-reduced where they are."""
        validdata = np.asarray(validdata)
        rank, world = 0, 1
        if distributed:
            own = getattr(self.tr, "dp_world", None)
            rank, world = own() if callable(own) else (0, 0)
            if world < 1:
                raise RuntimeError("a distributed resident demo cache is all-reduced on the device: the translator needs its own RCCL "
                                   "group (dp_init) -- or build it with resident=False over torch.distributed")
        self._resident_built = False
        for vp in range(self.nvp):
            ctx = np.ascontiguousarray(first_frames[vp], dtype=np.uint8)
            self.tr.reward_cache_begin(vp, self.batch_size)
            for _, u8 in self._demo_batches(validdata, rank, world):
                self.tr.reward_cache_add(vp, u8, ctx)
            self.tr.reward_cache_finish(vp, self._nvideos(validdata), distributed=distributed and world > 1)
        self._resident_built = True
        return self

    # ------------------------------------------------------------------ base.py:232-252
    def _costs_from(self, feats, frames_f32, vp):
        cf = np.sum((self.means[vp] - feats) ** 2, axis=1)
        ci = self.scale * np.sum((self.imgs[vp] - frames_f32) ** 2, axis=(1, 2, 3))
        if self.ablation_type == "nofeat":      # reference indexes self.imgs without [vp]
            return ci
        if self.ablation_type == "noimage":
            return cf
        return cf + ci

    def _group(self, distributed):
        """(rank, world, allsum) of the group a distributed call runs on: the translator's own RCCL group when it has one
        (Translator.dp_init -- ctx_dp_allreduce_host_f64, no torch in the sampler process), else an initialised torch.distributed group."""
        if not distributed:
            return 0, 1, (lambda x: x)
        own = getattr(self.tr, "dp_world", None)
        if callable(own) and own()[1] > 1:
            rank, world = own()
            return rank, world, self.tr.dp_allreduce_host
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()

        def allsum(x):
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
            if dist.get_backend() == "nccl":
                t = t.cuda()
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return t.cpu().numpy()
        return rank, world, (allsum if world > 1 else (lambda x: x))

    def paths_costs(self, paths, distributed=False):
        """costs[p][j] for every path, many paths per encoder launch.
        distributed=True (one rank per GPU, every rank holding the same `paths` and the same demo cache): the >= 250 rollout paths of a
        TRPO iteration are sharded rank::world -- a path's cost depends on nothing but its own frames (base.py:232-249) -- and the
        [npaths, bs] cost table is completed with ONE all-reduce (last sentence); every rank returns the full table."""
        rank, world, allsum = self._group(distributed)
        if world > 1:
            if self.means is None:
                raise RuntimeError("distributed paths_costs needs the demo cache first (build_demo_cache(..., distributed=True))")
            mine = list(range(rank, len(paths), world))
            part = np.zeros((len(paths), self.batch_size), np.float64)
            if mine:
                part[mine] = self.paths_costs([paths[i] for i in mine])
            return allsum(part.ravel()).reshape(part.shape).astype(np.float32)
        bs = self.batch_size
        frames = [self._frames_of(p) for p in paths]
        for f in frames:
            if len(f) != bs:
                raise ValueError(f"a path has {len(f)} rendered frames, the sampler's placeholder holds {bs} (base.py:115)")
        if self.means is None:
            if self.validdata is None:
                raise RuntimeError("no demo cache: call build_demo_cache(validdata, first_frames), or set_demos(validdata) to have it "
                                   "built on the first path like the reference (base.py:195-223)")
            # `context = imgs[0][vp]`: the first rendered frame of the FIRST path, per viewpoint (base.py:200)
            self.build_demo_cache(self.validdata, [frames[0][0][vp] for vp in range(self.nvp)])
        costs = np.zeros((len(paths), bs), np.float32)
        per_call = max(1, self.tr.max_batch // bs)
        for vp in range(self.nvp):
            for p0 in range(0, len(paths), per_call):
                grp = range(p0, min(len(paths), p0 + per_call))
                u8 = np.concatenate([np.stack([fr[vp] for fr in frames[p]]).astype(np.uint8) for p in grp])
                for p, c in zip(grp, self._group_costs(vp, u8, len(grp))):
                    # 'None' accumulates over viewpoints (costs += ...); the ablations overwrite (costs = ...)
                    costs[p] = costs[p] + c if self.ablation_type == "None" else c
        return costs

    def _group_costs(self, vp, u8, npaths):
        """costs [npaths, bs] of viewpoint vp for the uint8 frames [npaths * bs, ...] of one launch group, by the first route the
        hook and its translator allow."""
        tr, how = self.tr, (self.scale, self.ablation_type)
        if self.ablation_type == "recon":
            return self._group_costs_recon(vp, u8, npaths)
        if self.render_size is not None:
            rs = self._render.resizer()
            if hasattr(tr, "front") and self.resident:
                # raw frames up once -> f32 at the front end's size -> Mixed_7c -> encoder + cost; all on the front end's stream
                maps = tr.front.features_dev(rs.resize_dev(u8), u8.shape[0])
                return tr.tr.reward_costs_dev(vp, maps, npaths, *how)
            if not hasattr(tr, "front") and hasattr(tr, "reward_costs_dev"):
                # ... resized straight into the encoder's own frame slot (no device-to-device copy), then encoder + cost
                slot = tr.dev_frames(u8.shape[0])[0]
                return tr.reward_costs_dev(vp, rs.resize_dev(u8, dst=slot), npaths, *how)
            u8 = rs.resize(u8)                                             # no device cost entry: host uint8, then the routes below
        if self.resident:
            # every translator type: encoder (behind the front end in mode 'oursinception') + cost on the device
            return tr.reward_costs_u8(vp, u8, *how)
        if hasattr(tr, "reward_costs"):
            # encoder + cost on the device: only the [paths, bs] costs cross PCIe (not the 4-bytes-per-pixel frames)
            return tr.reward_costs(vp, u8, *how)
        feats, x = tr.encode(u8)                                           # [input_z, image_trans[0]], base.py:234-235
        bs = self.batch_size
        return np.stack([self._costs_from(feats[k * bs:(k + 1) * bs], x[k * bs:(k + 1) * bs], vp) for k in range(npaths)])

    def _group_costs_recon(self, vp, u8, npaths):
        """_group_costs for ablation_type='recon' (image_recon = out2), by the same routes in the same order."""
        tr = self.tr
        if self.render_size is not None:
            rs = self._render.resizer()
            if hasattr(tr, "front") and self.resident:
                maps = tr.front.features_dev(rs.resize_dev(u8), u8.shape[0])
                return tr.tr.reward_costs_recon_dev(vp, maps, npaths, self.scale)
            if not hasattr(tr, "front") and hasattr(tr, "reward_costs_recon_dev"):
                slot = tr.dev_frames(u8.shape[0])[0]
                return tr.reward_costs_recon_dev(vp, rs.resize_dev(u8, dst=slot), npaths, self.scale)
            u8 = rs.resize(u8)
        if self.resident:
            return tr.reward_costs_recon_u8(vp, u8, self.scale)
        if hasattr(tr, "reward_costs_recon"):
            return tr.reward_costs_recon(vp, u8, self.scale)
        # [input_z, out2] of base.py:234-235, every path in the context of its own first frame; image_trans[0] on the host
        recon, feats = tr.reconstruct(u8, None, npaths)
        if hasattr(tr, "front"):
            x = tr.encode(u8)[1]                                           # mode 'oursinception': image_trans IS the feature tensor (base.py:132)
        else:
            x = ((u8.astype(np.float32) * np.float32(1.0 / 255.0)) - np.float32(0.5)) * np.float32(2.0)  # base.py:116-119, three f32 operations
        bs = self.batch_size
        cf = np.sum((self.means[vp][None] - np.reshape(feats, (npaths, bs, -1))) ** 2, axis=2)
        ci = self.scale * np.sum(np.reshape(recon - x, (npaths, bs, -1)) ** 2, axis=2)
        return cf + ci

    # ------------------------------------------------------------------ base.py:256-257
    def process_paths(self, paths, distributed=False):
        """In place: path['rewards'][2j+1] -= costs[j] * j**2.  After set_demos(validdata) the demo cache is built lazily from
        the first path's first frame per viewpoint, as the reference does (base.py:195-200); otherwise build_demo_cache() must
        have been called.  distributed=True: the paths' costs are computed rank::world and gathered (paths_costs); every rank then
        applies them to its copy of `paths`."""
        if distributed and self.means is None and self.validdata is not None:
            frames0 = self._frames_of(paths[0])
            self.build_demo_cache(self.validdata, [frames0[0][vp] for vp in range(self.nvp)], distributed=True)
        costs = self.paths_costs(paths, distributed=distributed)
        apply_costs(paths, costs, self.batch_size)
        return costs


class InceptionFeatureReward:
    """The Inception-feature baseline of the reference's sampler (modes 'inception' / 'inceptionsame'; rllab/sampler/base.py:69-111
    to set up, :178-189 per path).  Per path: the 25 rendered frames of viewpoint 0 go through the frozen Inception-v3 up to `layer`,
      diff = means - feat;  diff[std == 0] = 0;  cost_j = mean over (h, w, c) of diff^2 / (std + 1e-5);  rewards[2j+1] -= cost_j * j^2.
    means / std [25, h, w, c] come from a meanfile ('inception': npz[layer], npz[layer + 'std']) or from expert rollouts
    ('inceptionsame': np.mean / np.std over axis 0 of their features).  Forward, statistics and cost run on the device
    (InceptionFrontend.stats / reward_costs); only the [paths, 25] costs cross PCIe.  `front` must be built with final=layer."""

    # how render-size frames reach the device: "block" = gathered into one array on the host and uploaded once, "list" = one upload
    # per frame from where the environment left it (FrameResizer's list form).  Measured (profiles/render_size_rewards.txt,
    # DESIGN.md section 10): equal at 25 frames, list 12 ms of 63 ms faster at 250 -- not a win at both counts, so the hook gathers;
    # an instance that always scores many paths per call may set `upload = "list"`.
    upload = "block"

    def __init__(self, front, layer, batch_size=25, paths_per_launch=None, render_size=None, resizer=None):
        """render_size=(Hr, Wr): env_infos['imgs'] (and the rollouts / videos of build_stats / build_meanfile) hold the frames as
        RENDERED, uint8 [Hr, Wr, 3]; the hook resizes them to the front end's size on the device (resize.FrameResizer on the front
        end's stream, max_frames = the frames of one forward): per forward the raw frames go up once, are resized to uint8 where the
        front end's conversion kernel reads them, and only the [paths, batch_size] costs (or the statistics) come back.  Results equal,
        bit for bit, those of a hook without render_size fed the same frames resized on the host.  Float frames are refused (imresize
        rescales floats by their range, which is not what the rollout does).  resizer: an object with resize(frames) (and, for the
        device chain, resize_u8_dev) to use instead of a FrameResizer; a front end without the device entries gets resizer.resize()
        followed by the host entry.  None (default): frames arrive at the front end's size, as before."""
        if layer == "Logits":
            raise ValueError("Logits is 2-D after TF's squeeze: the reference's mean over axes (1, 2, 3) is not defined on it")
        if getattr(front, "final", None) != layer:
            raise ValueError(f"the cost reads the front end's last end point: build it with final={layer!r} (got {getattr(front, 'final', None)!r})")
        self.front, self.layer, self.batch_size = front, layer, int(batch_size)
        self.paths_per_launch = int(paths_per_launch or max(1, front.max_images // self.batch_size))
        if self.batch_size > front.max_images:
            raise ValueError(f"a path's {self.batch_size} frames exceed the front end's max_images {front.max_images}")
        self.means, self.std = None, None
        # render_size -> the front end's frame size, on the front end's stream; holds the frames of one forward
        self._render = RenderFrames(render_size, lambda: ((front.H, front.W), self._per_forward() * self.batch_size,
                                                          getattr(front, "device", 0), front.stream), resizer)
        self.render_size = self._render.size

    _rs = property(lambda self: self._render.rs)                 # the resizer in use: the injected one, else a FrameResizer

    @classmethod
    def for_sampler(cls, mode, layer, imsize, meanfile=None, expert_rollouts=None, inception_ckpt=None, batch_size=25,
                    paths_per_launch=10, device=0, render_size=None):
        """What BaseSampler.initialize() sets up for mode.startswith('inception') (base.py:69-111): the front end on the sampler's
        imsize up to `layer` (variables from `inception_ckpt`, an .npz keyed by the TF names), and the statistics from `meanfile`
        (mode 'inception') or from the frames of expert rollouts (mode 'inceptionsame'; the reference rolls out 20).  render_size:
        the expert rollouts' and the paths' frames arrive as rendered (see __init__)."""
        from .inception_frontend import InceptionFrontend
        if mode not in ("inception", "inceptionsame"):
            raise ValueError(f"mode must be 'inception' or 'inceptionsame', got {mode!r}")
        # one forward holds as many whole paths as the front end's buffers allow (7 at 299 x 299); a launch of more is chunked
        per_forward = max(1, min(paths_per_launch, InceptionFrontend.max_images_limit(imsize[0], imsize[1], layer) // batch_size))
        front = InceptionFrontend(imsize[0], imsize[1], max_images=batch_size * per_forward, device=device, final=layer)
        if inception_ckpt is not None:
            front.load(inception_ckpt)
        r = cls(front, layer, batch_size=batch_size, paths_per_launch=paths_per_launch, render_size=render_size)
        if mode == "inception":
            if meanfile is None:
                raise ValueError("mode 'inception' reads its statistics from a meanfile")
            r.load_meanfile(meanfile)
        else:
            if expert_rollouts is None:
                raise ValueError("mode 'inceptionsame' builds its statistics from expert rollouts' frames")
            r.build_stats(expert_rollouts)
        return r

    # ------------------------------------------------------------------ frames as rendered
    def _per_forward(self):
        return max(1, self.front.max_images // self.batch_size)

    def _on_device(self):
        return self._render.on_device(self.front, "reward_costs_dev_u8")

    def _render_videos(self, videos):
        """videos of frames as rendered -> what front.stats takes: (videos, resize=) for the device chain, host-resized videos else."""
        videos = [list(v) for v in videos]
        for v in videos:
            self._render.check(v)
        rs = self._render.resizer()
        if self._on_device():
            return [gather([v], self.upload == "list") for v in videos], dict(resize=rs)
        return [rs.resize(gather([v])) for v in videos], {}

    # ------------------------------------------------------------------ statistics
    def set_stats(self, means, std):
        self.front.reward_set_stats(means, std)
        self.means, self.std = np.asarray(means, np.float32), np.asarray(std, np.float32)
        return self

    def load_meanfile(self, path):
        """data = np.load(meanfile); means = data[layer]; std = data[layer + 'std'] (base.py:107-109)."""
        with np.load(path) as z:
            return self.set_stats(z[self.layer], z[self.layer + "std"])

    def build_stats(self, rollouts):
        """rollouts: per expert rollout, its batch_size uint8 frames [H, W, 3] (viewpoint 0; base.py:94-105).  means / std are
        float32 np.mean / np.std over axis 0 of their features, bit for bit."""
        kw = {}
        if self.render_size is not None:
            rollouts, kw = self._render_videos(rollouts)
        (m, sd), = self.front.stats(rollouts, [self.layer], self.batch_size, **kw).values()
        return self.set_stats(m, sd)

    def build_meanfile(self, videos, layers, path=None):
        """The two-pass meanfile builder of the notebooks (per layer: sum over videos / count, then sum of (v - mean)^2 / count, sqrt;
        float32): one forward per video per pass through the front end for every end point in `layers` (at or before its `final`).  Writes
        {layer: means, layer + 'std': std} to `path` (np.savez) when given; returns the dict."""
        out, kw = {}, {}
        if self.render_size is not None:
            videos, kw = self._render_videos(videos)
        for name, (m, sd) in self.front.stats(videos, layers, self.batch_size, **kw).items():
            out[name], out[name + "std"] = m, sd
        if path is not None:
            np.savez(path, **out)
        return out

    # ------------------------------------------------------------------ base.py:178-189
    @staticmethod
    def _frames_of(path):
        """imgs = [img[0] for img in env_infos['imgs'] if img is not None]: viewpoint 0 of every rendered step (base.py:182)."""
        return [img[0] for img in path["env_infos"]["imgs"] if img is not None]

    def paths_costs(self, paths):
        """costs[p][j] for every path, paths_per_launch paths per device call."""
        if self.means is None:
            raise RuntimeError("no statistics: load_meanfile(path), build_stats(rollouts) or set_stats(means, std) first")
        bs = self.batch_size
        frames = [self._frames_of(p) for p in paths]
        for f in frames:
            if len(f) != bs:
                raise ValueError(f"a path has {len(f)} rendered frames, the sampler's placeholder holds {bs} (base.py:72)")
        costs = np.zeros((len(paths), bs), np.float32)
        per = self.paths_per_launch

        def score(grp):
            return self.front.reward_costs(gather(grp).astype(np.uint8, copy=False), len(grp))
        if self.render_size is not None:
            # frames as rendered: min(paths_per_launch, the paths of one forward) paths per call -- the resizer holds one forward's
            # frames -- each upload -> resize -> forward + cost on the front end's stream
            for f in frames:
                self._render.check(f)
            rs, per = self._render.resizer(), min(per, self._per_forward())
            if self._on_device():
                def score(grp):                                    # returns after the stream is drained
                    return self.front.reward_costs_dev_u8(rs.resize_u8_dev(gather(grp, self.upload == "list")), len(grp))
            else:
                def score(grp):
                    return self.front.reward_costs(rs.resize(gather(grp)), len(grp))
        for p0 in range(0, len(paths), per):
            grp = frames[p0:p0 + per]
            costs[p0:p0 + len(grp)] = score(grp)
        return costs

    def process_paths(self, paths):
        """In place: path['rewards'][2j+1] -= cost_j * j**2 (base.py:188-189).  Returns the costs."""
        costs = self.paths_costs(paths)
        apply_costs(paths, costs, self.batch_size)
        return costs


class ThirdPersonReward:
    """The two learned baselines of the comparison (launcher modes 'tpil' / 'gail'; sandbox/bradly/third_person/launchers/
    cyberpunk_aws.py, cyberpunk_aws_gail.py): a discriminator retrained every iteration on expert / on-policy (/ expert-fail)
    trajectories, whose P(expert) is the policy's reward.  Unlike the two classes above it is not frozen: every iteration calls
    set_data(...), train_cost(n_epochs) and then process_paths(paths) (third_person.ThirdPersonCost does the work on the device)."""
    N_EPOCHS = {"tpil": 10, "gail": 2}        # cyberpunk_trainer.py:113, cyberpunk_trainer_gail.py:83

    def __init__(self, cost, mode):
        self.cost, self.mode = cost, mode

    @classmethod
    def for_sampler(cls, mode, imsize, batch_size=32, device=0, seed=0, render_size=None):
        """render_size=(Hr, Wr): set_data's trajectories and the paths' im_observations hold frames as rendered, resized on the device
        (third_person.ThirdPersonCost)."""
        from .third_person import ConvDiscriminator, DomainConfusionVelocityDiscriminator, ThirdPersonCost
        if mode not in ("tpil", "gail"):
            raise ValueError(f"mode must be 'tpil' or 'gail', got {mode!r}")
        dim = [int(imsize[0]), int(imsize[1]), 3]
        disc = (DomainConfusionVelocityDiscriminator(dim, 2, 2, max_batch=batch_size, device=device, seed=seed) if mode == "tpil"
                else ConvDiscriminator(dim, max_batch=batch_size, device=device, seed=seed))
        return cls(ThirdPersonCost(disc, batch_size=batch_size, render_size=render_size), mode)

    def set_data(self, expert, on_policy, expert_fail=None):
        return self.cost.set_data(expert, on_policy, expert_fail)

    def train_cost(self, n_epochs=None):
        return self.cost.train_cost(self.N_EPOCHS[self.mode] if n_epochs is None else n_epochs)

    def process_paths(self, paths):
        """In place: path['rewards'] = P(expert) per frame (cyberpunk_rollout).  Returns the paths."""
        return self.cost.path_rewards(paths)
