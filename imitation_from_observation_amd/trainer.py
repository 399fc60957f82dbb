"""Translator training loop: `ModelTrainer` of scripts/train_script.py:28-204 over the HIP translator.

Same constructor arguments, same loop (`train_script.py:144-203`):
  * demo tensor vdata[T, N, H, W, 3] split into the first `ntrain` videos (training) and the rest (validation); the first
    200 training videos are written to `<basedir>vdata_train.npy` (:144-152);
  * for itr in 1 .. nitr-1: choicesrc, choicetgt = np.random.choice(ntrain, batch_size) twice;
    src[b] = traindata[b % nlen, choicesrc[b]], tgt[b] = traindata[b % nlen, choicetgt[b]], ctx[b] = traindata[0, choicetgt[b]];
    one Adam(1e-4) step; every 4th iteration logs "itr loss sim r1 r2 err" (:153-167);
  * every 40 iterations (and at every `save_every`) a validation batch sampled the same way from the held-out videos is
    evaluated and logged with a trailing "E" (:169-178);
  * every `save_every` iterations a checkpoint `<basedir><itr>/model_<itr>_<loss>_<r1>_<r2>_<err>` and `validloss.npy` are
    written, plus -- not for the Inception variant -- ten (translation, reconstruction) clips of single video pairs (:179-195);
  * from `save_every` on, every validation appends a row Iteration, Loss, Sim, R1, R2, NNErr to the tabular log (:196-203).

What differs, and why:
  * mp4 DECODING (:69, imageio + ffmpeg) is not available here: the demo tensor comes in as an array or a `.npy` path (the file
    the reference itself saves), or as `videos=` -- decoded videos [51, H, W, 3] uint8 -- which then go through the reference's own
    loop (:59-96: frame selection by nskip, `transform` = scipy.misc.imresize bilinear + /127.5 - 1, black-frame drop; restated in
    demo_pipeline.py, the resize bit-exact against Pillow; the list is shuffled with np.random first, :66) and are saved as
    `<basedir>vdata_strike<itr>.npy` like :95 (itr = the videos looked at);
  * the sess.run calls are `Translator.train_step_sampled` / `eval_sampled` on the demo tensor resident in HBM (uint8;
    `gather_triples_kernel` builds the batch with the trainer's x / 127.5 - 1 scaling) when the float demo tensor lies
    exactly on that uint8 lattice -- bit-identical to feeding the host-gathered float batch -- and
    `train_step` / `evaluate` on the host-gathered batch otherwise;
  * `nn_err` (:148) reads `featreshape`, which only exists in the Inception branch (NameError for the other
    models).  Its intended meaning -- for every output j the index of the nearest tgt frame, compared with j % nlen -- is
    computed on the host from `out` and the tgt slot for every model;
  * clips are written as `__<k>trans.gif` / `__<k>recon.gif` like :23-26, :193-194 -- by Pillow (imageio is absent), the frames
    `(clip(inverse_transform(f), 0, 1) * 255).astype(uint8)`; a box without Pillow gets the same frames as `.npy`;
  * the tabular log is a CSV `<basedir>progress.csv` (rllab's logger is outside the hot path).  As in the reference, on a
    save iteration its R1 / R2 columns hold the LAST CLIP's recon1 / recon2 (the clip loop re-uses the names, :192-193),
    while Loss / Sim / NNErr stay the validation batch's.
Random draws come from the global `np.random` in the reference's order, so a seeded run samples the same batches.

N GPUs (`rank`, `world`; new -- the reference is single-device): one ModelTrainer per process.  Every rank
keeps the whole uint8 demo tensor in HBM and runs the SAME loop: rank 0's `np.random` state is handed to the others once, so all
draw the same index arrays; `ctx_dp_train_step_sampled` gathers rank r's rows [r B/world, (r+1) B/world) of the GLOBAL batch on the
device (t = b % nlen on the global row b) and runs the bucketed RCCL step; the validation batch is sharded the same way
(`ctx_dp_eval_sampled`).  Logged scalars are GLOBAL (recon sums add, simloss is the mean over the global batch), `nn_err` is the sum
of the ranks' shares (each rank compares its outputs with ALL tgt frames of the batch), and only rank 0 writes checkpoints, clips,
`validloss.npy`, `vdata_train.npy` and the CSV.  The parameters after k steps equal the single-GPU run's on the same draws up to f32
summation order (tests/test_gpu_dp_two_ranks.py).
The Inception variant (`inception=True`) does the same with its uint8 frames resident in the front end: each rank gathers its rows
into the front end on the device (ctx_cnn_forward_sampled_dev), runs Inception on them per step as the reference graph does, and
trains the translator with ctx_dp_train_step on the maps; `nn_err` is ctx_dp_nn_err (the tgt maps are all-gathered on the devices,
never brought to the host).  On one GPU it keeps the host gather (train_step_u8 / evaluate_u8).

Gradient accumulation (`accum_steps=k`; new): the batch of every step is run in k micro-batches with ONE Adam update on the summed
gradient (`ctx_accum_train_step_sampled`, data parallel `ctx_dp_accum_train_step_sampled`: one all-reduce per step), so `batch_size`
may exceed what one launch sequence carries -- the model is created with max_batch = ceil(batch_size / world / k).  The draws, the
log, the CSV, checkpoints and clips are those of the same `batch_size` without accumulation, up to f32 summation order; `nn_err` of a
training batch is summed on the device.  Not for `inception=True`.
"""
from __future__ import annotations

import contextlib
import csv
import os

import numpy as np

from . import _lib

LEARNING_RATE = 1e-4          # fed at every step, train_script.py:163,167


def save_clip(stem, frames_u8):
    """savegif (train_script.py:22-26): one GIF of the uint8 frames [n, H, W, 3], 100 ms each, written by Pillow (which folds a frame equal
    to its predecessor into that one's display time: the animation is the same); `.npy` where Pillow is missing."""
    try:
        from PIL import Image
    except ImportError:
        np.save(stem, frames_u8)
        return stem + ".npy"
    ims = [Image.fromarray(np.ascontiguousarray(f)) for f in frames_u8]
    ims[0].save(stem + ".gif", save_all=True, append_images=ims[1:], loop=0, duration=100)
    return stem + ".gif"


def nn_err(tgt, out, nlen, j0=0):
    """train_script.py:148 with featreshape[2] = the tgt slot:
    sum_j | argmin_i mean((tgt_i - out_j)^2) - (j % nlen) |.
    j0: `out` holds rows j0, j0 + 1, ... of the batch (a data-parallel shard's share of the sum; `tgt` is always the whole batch)."""
    a = np.asarray(tgt, np.float64).reshape(len(tgt), -1)
    b = np.asarray(out, np.float64).reshape(len(out), -1)
    # mean((a_i - b_j)^2) = (|a_i|^2 + |b_j|^2 - 2 a_i.b_j) / n
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    return int(np.abs(np.argmin(d, axis=0) - (j0 + np.arange(len(out))) % nlen).sum())


def micro_slices(rows, accum_steps, first=0):
    """The micro-batches of an accumulated step: `rows` consecutive rows from `first` on in at most `accum_steps` slices [a, b) of
    ceil(rows / accum_steps) rows each -- the last may be short, and fewer slices come out when they cover the rows already.  Every
    row lies in exactly one slice."""
    if rows < 0 or accum_steps < 1:
        raise ValueError(f"rows = {rows}, accum_steps = {accum_steps}")
    micro = -(-rows // accum_steps)
    for a in range(0, rows, micro or 1):
        yield first + a, first + min(a + micro, rows)


def on_u8_lattice(vdata):
    """(uint8 tensor, True) when the float demo tensor is exactly what transform() makes of uint8 frames
    (k / 127.5 - 1, train_script.py:16-19), else (None, False)."""
    v = np.asarray(vdata)
    if v.dtype == np.uint8:
        return v, True
    k = np.rint((v.astype(np.float64) + 1.0) * 127.5)
    if k.min() < 0 or k.max() > 255:
        return None, False
    # exact: the f32 value the session is fed must BE the device table's entry  float32(k / 127.5 - 1)  (ctx_demos_upload)
    if not np.array_equal((k / 127.5 - 1.0).astype(np.float32), v.astype(np.float32)):
        return None, False
    return k.astype(np.uint8), True


TENSOR_STATS_COLUMNS = ("itr", "step", "applied", "name", "trainable", "g_norm", "g_rms", "g_absmax", "g_nonfinite", "p_norm", "p_absmax",
                        "p_nonfinite", "u_norm", "u_absmax", "update_ratio")


def check_tensor_stats_every(every):
    """The trainers' tensor_stats_every keyword: None, or an int >= 1 (ValueError otherwise, before anything touches a device)."""
    if every is None:
        return None
    if isinstance(every, bool) or int(every) != every or int(every) < 1:
        raise ValueError(f"tensor_stats_every = {every} must be an integer >= 1")
    return int(every)


def append_tensor_stats_csv(path, itr, stats):
    """One line per tensor of a Translator.tensor_stats() table, in param_info order, appended to `path` (TENSOR_STATS_COLUMNS)."""
    with open(path, "a", newline="") as f:
        w = csv.writer(f)
        for name, t in stats["tensors"].items():
            w.writerow([itr, stats["step"], int(stats["applied"]), name, int(t["trainable"])] + [repr(t[k]) for k in TENSOR_STATS_COLUMNS[5:]])


class ModelTrainer:
    MODELS = {"ContextSkipNew": "skipnew", "ContextAEReal": "real", "ContextAEInception": "inception2"}

    def __init__(self, idims, nvideos, ntrain, batch_size, model, nitr, save_every, nlen, nskip, rescale=True, inception=False,
                 strides=None, kernels=None, filters=None, *, vdata=None, basedir="model/", device=0, seed=0, translator=None,
                 precision=None, log=print, rank=0, world=1, dp_unique_id=None, videos=None, device_resize=False,
                 grad_clip=None, skip_nonfinite=False, var_list=None, lr_scales=None, weight_decay=None, lr_schedule=None, tensor_stats_every=None,
                 ema_decay=None, ema_eval=False, accum_steps=1):
        """The reference's 14 positional arguments (train_script.py:29-30; the launchers omit the last five, SURVEY.md 3.4-b,
        hence the defaults), then: vdata (array or .npy path of the demo tensor), basedir (logger._snapshot_dir), device,
        seed of the parameter initialiser, an optional ready-made translator (tests), the arithmetic (precision: "f32" | "bf16x3" | "fp16x3" | "fp16x3d",
        Translator.__init__; None = its default), the log sink.
        rank / world: one trainer per GPU process (module docstring); `batch_size` stays the GLOBAL batch (a multiple of world).
        dp_unique_id: the 128-byte blob of Translator.dp_unique_id() made on rank 0 and shipped to every rank by the launcher (omitted:
        broadcast through an initialised torch.distributed group; not needed when `translator` already went through dp_init).
        device_resize: with `videos=`, the demo frames are resized on the device (demo_pipeline.device_resize: the same bytes as the
        host resize, one call per video) instead of on the host.
        grad_clip / skip_nonfinite: Translator.set_grad_guard -- clip every step's gradient by its global norm (data parallel: of the
        reduced gradient), leave parameters and Adam moments untouched on a step whose gradient is non-finite (one extra log line
        then).  Defaults: no guard, logs and checkpoints as without these keywords.
        var_list / lr_scales: which variables Adam trains (`minimize(loss, var_list=...)`, train_script.py:126-128).  var_list: fnmatch
        patterns on the TF variable names ("deconv/*") -- Translator.set_trainable, everything else is frozen; lr_scales: {pattern:
        scale} -- Translator.set_lr_scales.  One of the two; set once before the first step.  Defaults: every variable, as before.
        tensor_stats_every: k >= 1 takes per-tensor gradient, parameter and update statistics on the device behind every k-th Adam
        update (Translator.set_tensor_stats, two extra launches then) and appends one line per tensor to `<basedir>tensor_stats.csv`
        (TENSOR_STATS_COLUMNS, no header line; rank 0 only), and with skip_nonfinite the log line of a skipped step names the tensors
        whose gradient held non-finite elements.  Default: none; logs, CSV and checkpoints as before.
        ema_decay: a decay in [0, 1) keeps an exponential moving average of the parameters on the device (Translator.set_ema with the
        warm-up schedule, one extra launch per Adam update) and writes, at every `save_every`, a second file `model_ema_<itr>` beside
        the usual checkpoint: the AVERAGED weights under the variable names (Translator.save(weights="ema")), which the reward hook
        loads like any checkpoint.  ema_eval=True (needs ema_decay) runs the validation batch and the clips of a `save_every`
        iteration on the averaged weights (one extra log line then).  Defaults: no average; logs, CSV, checkpoints and draws as before.
        accum_steps: k > 1 steps every batch in k micro-batches with ONE Adam update on the summed gradient
        (Translator.train_step_sampled_accum; data parallel: dp_train_step_sampled_accum, one all-reduce per step).  `batch_size` stays
        the GLOBAL batch and the draws from np.random are those of a trainer with that batch_size; the model is created with
        max_batch = ceil(batch_size / world / k), so the batch no longer has to fit one launch sequence.  Logs, progress.csv,
        checkpoints and clips are as before (validation batches are evaluated in the same slices and their scalars combined).
        Needs the device-resident sampler (a demo tensor on the uint8 lattice).  Out of scope: inception=True -- the front end would
        have to run on every tgt frame first for the global nn_err -- which raises ValueError.  Default 1: the code path as before.
        weight_decay: decoupled weight decay (AdamW) inside the fused Adam pass -- Translator.set_weight_decay: a float lambda for every
        kernel and matrix (not the biases) or {pattern: lambda}; set once before the first step, beside the mask.  Default: none; logs,
        files and draws as before.
        lr_schedule: a callable itr -> learning rate used in place of the constant 1e-4 (train_script.py:163,167) at iteration itr
        (from 1); a negative or non-finite value raises before that step.  The decay per step is lr * lambda, so it follows the
        schedule by itself.  Default: the constant rate."""
        if model not in self.MODELS:
            raise ValueError(f"model must be one of {sorted(self.MODELS)}")
        self.idims, self.nvideos, self.ntrain, self.batch_size = tuple(idims), nvideos, ntrain, batch_size
        self.model, self.nitr, self.save_every, self.nlen, self.nskip = model, nitr, save_every, nlen, nskip
        self.rescale, self.inception = rescale, inception
        self.strides, self.kernels, self.filters = strides, kernels, filters
        self.vdata, self.basedir, self.device, self.seed = vdata, basedir, device, seed
        self.device_resize = bool(device_resize)
        self.grad_clip, self.skip_nonfinite = grad_clip, bool(skip_nonfinite)
        if var_list is not None and lr_scales is not None:
            raise ValueError("var_list and lr_scales are two spellings of one mask: give one")
        self.var_list, self.lr_scales = var_list, lr_scales
        if lr_schedule is not None and not callable(lr_schedule):
            raise ValueError("lr_schedule must be a callable itr -> learning rate")
        self.weight_decay, self.lr_schedule = weight_decay, lr_schedule
        self.videos = videos       # decoded demo videos (arrays [51, H, W, 3] uint8 or callables returning them): train_script.py:59-96
        self.translator, self.precision, self.log = translator, precision, log
        self.rank, self.world, self.dp_unique_id = int(rank), int(world), dp_unique_id
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"rank {rank} / world {world}")
        if self.world > 1 and batch_size % self.world:
            raise ValueError(f"batch_size {batch_size} (the GLOBAL batch) must be a multiple of world = {world}")
        self.tensor_stats_every = check_tensor_stats_every(tensor_stats_every)
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay = {ema_decay} must lie in [0, 1)")
        if ema_eval and ema_decay is None:
            raise ValueError("ema_eval=True evaluates on the averaged weights: give ema_decay")
        self.ema_decay, self.ema_eval = (None if ema_decay is None else float(ema_decay)), bool(ema_eval)
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError(f"accum_steps = {accum_steps}")
        if self.accum_steps > 1 and inception:
            raise ValueError("accum_steps > 1 is not available with inception=True: its front end would have to run on every tgt frame "
                             "of the batch first (Translator.accum_begin .. accum_adam work on device maps)")
        self.allloss, self.validloss = [], []

    # ------------------------------------------------------------------ the model behind the four sess.run sites
    def _build(self):
        if self.translator is not None:
            return self.translator
        from .translator import Translator
        H, W = self.idims
        if self.inception:
            from .oursinception import InceptionTranslator
            tr = InceptionTranslator((H, W), max_batch=self.batch_size // self.world, device=self.device, precision=self.precision,
                                     strides=self.strides, kernels=self.kernels, filters=self.filters)   # train_script.py:110
            tr.tr.init_params(self.seed)
            return tr
        variant = self.MODELS[self.model]
        tr = Translator(H, W, featsize=100 if variant == "real" else 1024, max_batch=-(-(self.batch_size // self.world) // self.accum_steps),
                        device=self.device, variant=variant, precision=self.precision)
        tr.init_params(self.seed)                                  # tf.global_variables_initializer, train_script.py:129
        return tr

    def _join_group(self, tr):
        """world > 1: this rank's handle joins the RCCL group (ctx_dp_init: rank 0's parameters / Adam state reach every replica)."""
        if tr.dp_world()[1] == self.world:
            return
        uid = self.dp_unique_id
        if uid is None:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("world > 1 needs dp_unique_id (Translator.dp_unique_id() of rank 0) or an initialised torch.distributed group")
            box = [type(tr).dp_unique_id() if self.rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            uid = box[0]
        tr.dp_init(uid, self.rank, self.world)

    def _batch(self, data, choicesrc, choicetgt):
        ar = np.arange(0, self.batch_size) % self.nlen
        return data[ar, choicesrc], data[0, choicetgt], data[ar, choicetgt]          # srcdata, tgtctx, tgtdata (:156-159)

    def train(self):
        basedir = self.basedir if self.basedir.endswith("/") else self.basedir + "/"
        os.makedirs(basedir, exist_ok=True)
        rank, world, dp = self.rank, self.world, self.world > 1
        tr = self._build()
        if dp:
            self._join_group(tr)

        def allsum(x):
            """sum over the ranks of a small host array (ctx_dp_allreduce_host_f64); the identity on one GPU"""
            x = np.ascontiguousarray(x, dtype=np.float64)
            return tr.dp_allreduce_host(x) if dp else x
        if dp:
            # every rank draws the same numbers: rank 0's np.random state (MT19937: 624 words + position + the cached gaussian) --
            # BEFORE build_vdata, whose np.random.shuffle(videos) decides the video order, the subset and the train / valid split
            st = np.random.get_state()
            flat = np.zeros(627, np.float64)
            if rank == 0:
                flat[:624], flat[624], flat[625], flat[626] = st[1], st[2], st[3], st[4]
            flat = allsum(flat)
            np.random.set_state((st[0], flat[:624].astype(np.uint32), int(flat[624]), int(flat[625]), float(flat[626])))
        if self.vdata is None and self.videos is not None:
            from .demo_pipeline import build_vdata, device_resize
            vdata, looked_at = build_vdata(self.videos, self.idims, self.nvideos, self.nlen, self.nskip, self.rescale, self.inception,
                                           log=self.log if self.rank == 0 else None, return_count=True,
                                           resize=device_resize(self.device) if self.device_resize else None)
            if self.rank == 0:
                np.save(basedir + "vdata_strike" + str(looked_at), vdata)                      # train_script.py:95 (named after `itr`, the videos looked at)
        else:
            vdata = np.load(self.vdata) if isinstance(self.vdata, (str, os.PathLike)) else np.asarray(self.vdata)
        if vdata.ndim != 5 or vdata.shape[2:4] != self.idims or vdata.shape[0] < self.nlen:
            raise ValueError(f"vdata must be [T >= {self.nlen}, N, {self.idims[0]}, {self.idims[1]}, 3], got {vdata.shape}")
        B, nlen = self.batch_size, self.nlen
        log = self.log if rank == 0 else (lambda s: None)          # one log, one set of files: rank 0's
        if not (self.vdata is None and self.videos is not None):
            log(str(vdata.shape))                                  # (:96 -- build_vdata logs it on the `videos=` path)
        Bl, j0 = B // world, rank * (B // world)                   # this rank's rows of the global batch
        n = vdata.shape[1]
        ntrain = self.ntrain
        nvalid = n - ntrain
        if ntrain <= 0 or nvalid <= 0:
            raise ValueError(f"ntrain = {ntrain} of {n} videos leaves no training / validation split")
        log("%s %s" % (ntrain, nvalid))
        validdata = vdata[:, ntrain:]
        traindata = vdata[:, :ntrain]
        log(str(validdata.shape) + str(traindata.shape))
        if rank == 0:
            np.save(basedir + "vdata_train", traindata[:, :200])
        # device-resident demo tensor + device sampler where that is bit-identical to the host gather.  The Inception variant feeds
        # uint8 frames to its front end: data parallel it samples them on the device (the front end's sampler), on one GPU it keeps
        # the host gather
        if self.inception:
            u8 = vdata if vdata.dtype == np.uint8 else None
            resident = dp and u8 is not None
            if dp and not resident:
                raise ValueError("data-parallel Inception training samples on the device: the demo tensor must be the uint8 frames "
                                 f"(got {vdata.dtype})")
        else:
            u8, lattice = on_u8_lattice(vdata)
            resident = lattice and hasattr(tr, "load_demos")
        if dp and not resident:
            raise ValueError("data-parallel training runs on the device-resident sampler: the demo tensor must lie on the uint8 lattice "
                             "(k / 127.5 - 1, what train_script.py:16-19 makes of video frames)")
        if resident:
            # only frames t < nlen are ever sampled (t = b % nlen, and frame 0 for the context); the device sampler takes
            # t = b % T with T = the uploaded tensor's length, so upload exactly nlen frames (vdata may hold more)
            try:
                tr.load_demos(np.ascontiguousarray(u8[:nlen]))
            except Exception as e:
                if self.inception and getattr(e, "code", None) == _lib.CTX_E_NOMEM:
                    raise ValueError(f"data-parallel Inception training keeps the demo tensor {u8[:nlen].shape} resident on every rank "
                                     f"and it does not fit on the device ({e}): fewer videos, or one GPU (host gather)") from e
                raise
        dp_incep = dp and self.inception                           # nn_err of the global batch on the device (ctx_dp_nn_err)
        accum = self.accum_steps > 1
        if accum and not resident:
            raise ValueError("accum_steps > 1 steps through the device-resident sampler: the demo tensor must lie on the uint8 lattice "
                             "(k / 127.5 - 1, what train_script.py:16-19 makes of video frames)")
        micro = -(-Bl // self.accum_steps)                         # rows of a micro-batch (the last may be short: micro_slices)

        def train_step(cs, ct, want_err=False, lr=LEARNING_RATE):
            if accum:                                              # GLOBAL scalars, and nn_err of the whole batch from the device
                step = tr.dp_train_step_sampled_accum if dp else tr.train_step_sampled_accum
                return step(cs, ct, micro, lr=lr, nlen=nlen if want_err else None)
            if dp:
                return tr.dp_train_step_sampled(cs, ct, lr=lr)                     # GLOBAL scalars
            if resident:
                return tr.train_step_sampled(cs, ct, lr=lr)
            src, ctx, tgt = self._batch(traindata, cs, ct)
            if self.inception:
                return tr.train_step_u8(src, ctx, tgt, lr=lr)
            return tr.train_step(src, ctx, tgt, lr=lr)

        def lr_at(itr):
            if self.lr_schedule is None:
                return LEARNING_RATE
            lr = float(self.lr_schedule(itr))
            if not (np.isfinite(lr) and lr >= 0.0):
                raise ValueError(f"lr_schedule({itr}) = {lr}: the learning rate must be finite and >= 0")
            return lr

        def evaluate(cs, ct):
            """loss, sim, r1, r2, out, out2, tgt of a validation batch (indices into validdata)."""
            if dp_incep:                                       # GLOBAL scalars; nn_err is taken on the device (dp_nn_err)
                return tr.dp_eval_sampled(np.asarray(cs) + ntrain, np.asarray(ct) + ntrain, outputs=False), None
            src, ctx, tgt = self._batch(validdata, cs, ct)
            if accum:                                          # the batch does not fit the handle: this rank's rows in the step's slices
                parts = [(b - a, tr.evaluate(src[a:b], ctx[a:b], tgt[a:b])) for a, b in micro_slices(Bl, self.accum_steps, j0)]
                # recon sums add, simloss is the mean over the GLOBAL batch, `loss` the terms the model keeps (as ctx_dp_scalars)
                sim, r1, r2 = allsum([sum(p["simloss"] * n for n, p in parts) / B, sum(p["recon1"] for _, p in parts),
                                      sum(p["recon2"] for _, p in parts)])
                terms = int(getattr(getattr(tr, "cfg", None), "loss_terms", 0) or 0) or 7
                loss = (r1 if terms & 1 else 0.0) + (r2 if terms & 2 else 0.0) + (sim if terms & 4 else 0.0)
                return dict(loss=float(loss), simloss=float(sim), recon1=float(r1), recon2=float(r2),
                            out=np.concatenate([p["out"] for _, p in parts]), out2=np.concatenate([p["out2"] for _, p in parts])), tgt
            if dp:                                             # GLOBAL scalars; out / out2 = this rank's rows
                ev = tr.dp_eval_sampled(np.asarray(cs) + ntrain, np.asarray(ct) + ntrain)
            elif resident:
                ev = tr.eval_sampled(np.asarray(cs) + ntrain, np.asarray(ct) + ntrain)
            elif self.inception:                               # feature maps stay on the device; nn_err compares with the tgt MAPS
                ev = tr.evaluate_u8(src, ctx, tgt)
                tgt = ev["tgt"]
            else:
                ev = tr.evaluate(src, ctx, tgt)
            return ev, tgt

        core = getattr(tr, "tr", tr)                               # the Translator inside an InceptionTranslator
        guarded = self.grad_clip is not None or self.skip_nonfinite
        if guarded:
            core.set_grad_guard(self.grad_clip, self.skip_nonfinite)
        if self.var_list is not None:
            core.set_trainable(self.var_list)
        elif self.lr_scales is not None:
            core.set_lr_scales(self.lr_scales)
        if self.weight_decay is not None:
            core.set_weight_decay(self.weight_decay)
        if self.ema_decay is not None:
            core.set_ema(self.ema_decay)
        if self.tensor_stats_every is not None:
            core.set_tensor_stats(self.tensor_stats_every)
        stats_step = None                                      # the Adam step of the last table written
        skipped = 0
        rows = []
        for itr in range(1, self.nitr):
            choicesrc = np.random.choice(ntrain, B)
            choicetgt = np.random.choice(ntrain, B)
            sc = train_step(choicesrc, choicetgt, want_err=itr % 4 == 0, lr=lr_at(itr))
            if self.tensor_stats_every is not None and rank == 0 and itr % self.tensor_stats_every == 0:
                st = core.tensor_stats()                       # (the table the step left behind its update; an on-demand one has no update)
                if st["has_update"] and st["step"] != stats_step:
                    stats_step = st["step"]
                    append_tensor_stats_csv(basedir + "tensor_stats.csv", itr, st)
            if guarded and self.skip_nonfinite:                # (the step has synchronised for its scalars: the counters are final)
                now = core.guard_stats()["steps_skipped"]
                if now > skipped:
                    skipped = now
                    msg = "%s skipped: non-finite gradient, parameters and Adam moments unchanged (%s so far)" % (itr, skipped)
                    if self.tensor_stats_every is not None and rank == 0:      # the gradient arena still holds the offending gradient
                        bad = [n for n, t in core.tensor_stats(compute="grads")["tensors"].items() if t["g_nonfinite"] > 0]
                        msg += "; non-finite in: " + (", ".join(bad) if bad else "none of the trainable tensors")
                    log(msg)
            if itr % 4 == 0:
                if accum:                                      # summed over the micro-batches on the device
                    err = sc["nn_err"]
                elif dp_incep:                                 # the tgt maps exist only on the device, one shard per rank
                    err = int(tr.dp_nn_err(nlen))
                else:
                    out, _, tgt = core.last_outputs(out=True, tgt=True)
                    if dp:                                     # this rank's outputs against ALL tgt frames of the batch (:148)
                        tgt = self._batch(traindata, choicesrc, choicetgt)[2]
                    err = int(allsum([nn_err(tgt, out, nlen, j0)])[0])
                log("%s %s %s %s %s %s" % (itr, sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"], err))
                self.allloss.append(sc["loss"])
            if itr % 40 == 0 or itr % self.save_every == 0:
                choicesrc = np.random.choice(nvalid, B)
                choicetgt = np.random.choice(nvalid, B)
                on_ema = self.ema_eval and itr % self.save_every == 0      # this iteration's validation and clips on the averaged weights
                if on_ema:
                    log("%s validation and clips on the averaged weights (decay %s, %s updates)" % (itr, self.ema_decay, core.ema_state()["updates"]))
                with core.ema_weights() if on_ema else contextlib.nullcontext():
                    ev, tgt = evaluate(choicesrc, choicetgt)
                loss, sim, r1, r2 = ev["loss"], ev["simloss"], ev["recon1"], ev["recon2"]
                err = int(tr.dp_nn_err(nlen)) if dp_incep else int(allsum([nn_err(tgt, ev["out"], nlen, j0)])[0])
                log("%s %s %s %s %s %s E" % (itr, loss, sim, r1, r2, err))
                self.validloss.append(loss)
                if itr % self.save_every == 0:
                    if rank == 0:
                        os.mkdir(basedir + str(itr))
                        core.save("%s%d/model_%d_%.2f_%.2f_%.2f_%d" % (basedir, itr, itr, loss, r1, r2, err), prefix="contextmodel/")
                        if self.ema_decay is not None:         # the inference checkpoint of the averaged weights, beside it
                            core.save("%s%d/model_ema_%d" % (basedir, itr, itr), prefix="contextmodel/", weights="ema")
                        np.save("%s%d/validloss" % (basedir, itr), self.validloss)
                    if not self.inception:
                        with core.ema_weights() if on_ema else contextlib.nullcontext():
                            for kk in range(10):
                                choicesrc = [np.random.randint(nvalid)] * B
                                choicetgt = [np.random.randint(nvalid)] * B
                                clip, _ = evaluate(choicesrc, choicetgt)
                                r1, r2 = clip["recon1"], clip["recon2"]           # the reference's clip fetch overwrites r1 / r2 (:192-193): the
                                                                                  # tabular R1 / R2 of a save iteration are the last clip's
                                for tag, frames in (("trans", clip["out"]), ("recon", clip["out2"])):
                                    if dp:                         # the clip is rows 0 .. nlen-1 of the GLOBAL batch: every rank adds the rows it holds
                                        head = np.zeros((nlen,) + frames.shape[1:], np.float64)
                                        lo, hi = max(j0, 0), min(j0 + Bl, nlen)
                                        if hi > lo:
                                            head[lo:hi] = frames[lo - j0:hi - j0]
                                        # (the group sums in float64; the quantisation below is the single-GPU path's and the reference's float32 arithmetic)
                                        frames = allsum(head.ravel()).reshape(head.shape).astype(np.float32)
                                    u = (np.clip((frames[:nlen] + 1.0) / 2.0, 0, 1) * 255).astype(np.uint8)     # savegif's frames (:23-26)
                                    if rank == 0:
                                        save_clip("%s%d/__%d%s" % (basedir, itr, kk, tag), u)
                if itr >= self.save_every and rank == 0:
                    rows.append(dict(Iteration=itr, Loss=loss, Sim=sim, R1=r1, R2=r2, NNErr=err))
                    with open(basedir + "progress.csv", "w", newline="") as f:
                        w = csv.DictWriter(f, fieldnames=["Iteration", "Loss", "Sim", "R1", "R2", "NNErr"])
                        w.writeheader()
                        w.writerows(rows)
        self.translator = tr
        return tr
