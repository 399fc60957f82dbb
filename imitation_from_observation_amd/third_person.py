"""The third-person-imitation ('tpil') and GAIL ('gail') baseline rewards of the reference's comparison: the two discriminators of
sandbox/bradly/third_person/discriminators/discriminator.py with the reference's method names, and the cost-training loop of
algos/cyberpunk_trainer.py / cyberpunk_trainer_gail.py on a device-resident data set.

All arithmetic runs in libctxtrans.so (ctx_disc_* of include/ctxtrans.h; kernels in csrc/disc.hip); this file is numpy + ctypes only.
Frames are raw pixel values 0..255, [B, H, W, 3], float32 or uint8 -- the reference feeds imresize output without any scaling."""
import ctypes

import numpy as np

from . import _lib
from ._lib import CTX_DISC_GAIL, CTX_DISC_TPIL, CtxDiscConfig, CtxError
from .render_frames import RenderFrames, gather

_F = ctypes.POINTER(ctypes.c_float)
_U8 = ctypes.POINTER(ctypes.c_uint8)
_I32 = ctypes.POINTER(ctypes.c_int32)


def _fp(a):
    return a.ctypes.data_as(_F)


class _Discriminator:
    """Common host side of the two discriminators: one ctx_disc handle."""
    variant = None
    learning_rate = 0.001            # Discriminator.__init__ (discriminator.py:11)

    def __init__(self, input_dim, max_batch=32, device=0, seed=0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.input_dim = tuple(int(d) for d in input_dim)
        self.H, self.W, C = self.input_dim
        self.max_batch, self.device = int(max_batch), int(device)
        cfg = CtxDiscConfig(variant=self.variant, H=self.H, W=self.W, C=C, max_batch=self.max_batch)
        rc = self._lib.ctx_disc_create(ctypes.byref(cfg), int(device), ctypes.byref(self._h))
        if rc != _lib.CTX_OK:
            msg = self._lib.ctx_disc_last_error(None)
            self._h = ctypes.c_void_p()
            raise CtxError(rc, msg.decode() if msg else "")
        self._names = []
        name, ndim = ctypes.c_char_p(), ctypes.c_int()
        shape, off = (ctypes.c_int64 * 4)(), ctypes.c_int64()
        for i in range(self._lib.ctx_disc_param_count(self._h)):
            self._ck(self._lib.ctx_disc_param_info(self._h, i, ctypes.byref(name), ctypes.byref(ndim), shape, ctypes.byref(off)))
            self._names.append((name.value.decode(), tuple(shape[:ndim.value]), off.value))
        self.param_total = sum(int(np.prod(s)) for _, s, _ in self._names)
        self._ck(self._lib.ctx_disc_init_params(self._h, int(seed)))

    # ------------------------------------------------------------------ plumbing
    @classmethod
    def param_total_for(cls, input_dim, max_batch=32):
        cfg = CtxDiscConfig(variant=cls.variant, H=int(input_dim[0]), W=int(input_dim[1]), C=int(input_dim[2]), max_batch=int(max_batch))
        n = _lib.load().ctx_disc_param_total_for(ctypes.byref(cfg))
        if n < 0:
            raise CtxError(int(n), _lib.load().ctx_disc_last_error(None).decode())
        return int(n)

    def _ck(self, rc):
        if rc != _lib.CTX_OK:
            msg = self._lib.ctx_disc_last_error(self._h)
            raise CtxError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ctx_disc_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _split(self, flat):
        return {n: flat[o:o + int(np.prod(s))].reshape(s).copy() for n, s, o in self._names}

    def _join(self, params):
        flat = np.empty(self.param_total, np.float32)
        for n, s, o in self._names:
            a = np.asarray(params[n], np.float32)
            if a.shape != s:
                raise ValueError(f"{n}: shape {a.shape}, expected {s}")
            flat[o:o + a.size] = a.ravel()
        return flat

    def _get(self, fn):
        flat = np.empty(self.param_total, np.float32)
        self._ck(fn(self._h, _fp(flat), flat.size))
        return flat

    def get_params(self):
        return self._split(self._get(self._lib.ctx_disc_get_params))

    def get_grads(self):
        return self._split(self._get(self._lib.ctx_disc_get_grads))

    def set_params(self, params):
        flat = self._join(params)
        self._ck(self._lib.ctx_disc_set_params(self._h, _fp(flat), flat.size))

    def get_adam_state(self):
        m, v = np.empty(self.param_total, np.float32), np.empty(self.param_total, np.float32)
        t = ctypes.c_int64()
        self._ck(self._lib.ctx_disc_get_adam_state(self._h, _fp(m), _fp(v), m.size, ctypes.byref(t)))
        return self._split(m), self._split(v), t.value

    def set_adam_state(self, m, v, step):
        fm, fv = self._join(m), self._join(v)
        self._ck(self._lib.ctx_disc_set_adam_state(self._h, _fp(fm), _fp(fv), fm.size, int(step)))

    def init_params(self, seed):
        self._ck(self._lib.ctx_disc_init_params(self._h, int(seed)))

    def save(self, path):
        """Parameters by name into an .npz (the extension is added when missing, as np.savez does)."""
        np.savez(path, **self.get_params())

    def load(self, path):
        path = str(path)
        with np.load(path if path.endswith(".npz") else path + ".npz") as z:
            self.set_params({n: z[n] for n, _, _ in self._names})

    def debug_read(self, name, n):
        out = np.empty(int(n), np.float32)
        self._ck(self._lib.ctx_disc_debug_read(self._h, name.encode(), _fp(out), out.size))
        return out

    # ------------------------------------------------------------------ batches
    def _pair(self, data):
        """data = [x1, x2] (TPIL) or [x, time] (GAIL) -> contiguous arrays, the u8 flag and B."""
        if len(data) != 2:
            raise ValueError("data batch should have length two")
        x1 = np.asarray(data[0])
        u8 = x1.dtype == np.uint8
        x1 = np.ascontiguousarray(x1, np.uint8 if u8 else np.float32)
        if x1.ndim != 4 or x1.shape[1:] != (self.H, self.W, 3):
            raise ValueError(f"frames {x1.shape}, expected [B, {self.H}, {self.W}, 3]")
        if self.variant == CTX_DISC_TPIL:
            x2 = np.ascontiguousarray(data[1], x1.dtype)
            if x2.shape != x1.shape:
                raise ValueError(f"second frames {x2.shape}, expected {x1.shape}")
        else:
            x2 = np.ascontiguousarray(np.asarray(data[1], np.float32).reshape(-1))
            if x2.shape[0] != x1.shape[0]:
                raise ValueError(f"time column {x2.shape}, expected {x1.shape[0]} rows")
        return x1, x2, u8, x1.shape[0]

    def _chunks(self, B):
        return range(0, B, self.max_batch)

    def _logits(self, data, softmax):
        x1, x2, u8, B = self._pair(data)
        out = np.empty((B, 2), np.float32)
        fn = self._lib.ctx_disc_logits_u8 if u8 else self._lib.ctx_disc_logits
        for b0 in self._chunks(B):
            b1 = min(B, b0 + self.max_batch)
            a, b, o = x1[b0:b1], x2[b0:b1], out[b0:b1]
            self._ck(fn(self._h, a.ctypes.data_as(_U8 if u8 else _F), b.ctypes.data_as(ctypes.c_void_p if u8 else _F), b1 - b0,
                        1 if softmax else 0, _fp(o)))
        return out

    def _train(self, data, classes, domains):
        x1, x2, u8, B = self._pair(data)
        cls = np.ascontiguousarray(classes, np.float32).reshape(B, 2)
        dom = None if domains is None else np.ascontiguousarray(domains, np.float32).reshape(B, 2)
        loss = ctypes.c_float()
        fn = self._lib.ctx_disc_train_u8 if u8 else self._lib.ctx_disc_train
        self._ck(fn(self._h, x1.ctypes.data_as(_U8 if u8 else _F), x2.ctypes.data_as(ctypes.c_void_p if u8 else _F), _fp(cls),
                    None if dom is None else _fp(dom), B, self.learning_rate, ctypes.byref(loss)))
        return np.float32(loss.value)

    def _accuracy(self, data, class_labels):
        x1, x2, u8, B = self._pair(data)
        cls = np.ascontiguousarray(class_labels, np.float32).reshape(B, 2)
        acc = ctypes.c_float()
        fn = self._lib.ctx_disc_accuracy_u8 if u8 else self._lib.ctx_disc_accuracy
        self._ck(fn(self._h, x1.ctypes.data_as(_U8 if u8 else _F), x2.ctypes.data_as(ctypes.c_void_p if u8 else _F), _fp(cls), B,
                    ctypes.byref(acc)))
        return np.float32(acc.value)

    def __call__(self, data, softmax=True):
        return self._logits(data, softmax)

    def get_reward(self, data, softmax=True):
        return self._logits(data, softmax)

    # ------------------------------------------------------------------ resident forms
    def data_upload(self, frames, classes, domains=None):
        """frames uint8 [N, T, H, W, 3]; classes / domains one-hot [N, 2] per trajectory."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim != 5 or frames.shape[2:] != (self.H, self.W, 3):
            raise ValueError(f"frames {frames.shape}, expected [N, T, {self.H}, {self.W}, 3]")
        N, T = frames.shape[:2]
        cls = np.ascontiguousarray(classes, np.float32).reshape(N, 2)
        dom = None if domains is None else np.ascontiguousarray(domains, np.float32).reshape(N, 2)
        self._ck(self._lib.ctx_disc_data_upload(self._h, frames.ctypes.data_as(_U8), N, T, _fp(cls), None if dom is None else _fp(dom)))

    def train_epoch(self, order, batch=32, shift=3, with_accuracy=True, lr=None):
        """One pass over the resident rows `order` (flat trajectory * T + t) in slices of `batch`; returns (losses, accuracies) per batch
        (accuracies None without with_accuracy)."""
        order = np.ascontiguousarray(order, np.int32)
        nb = -(-order.size // int(batch))
        losses = np.empty(nb, np.float32)
        accs = np.empty(nb, np.float32) if with_accuracy else None
        self._ck(self._lib.ctx_disc_train_epoch(self._h, order.ctypes.data_as(_I32), order.size, int(batch), int(shift),
                                                self.learning_rate if lr is None else float(lr), 1 if with_accuracy else 0, _fp(losses),
                                                None if accs is None else _fp(accs)))
        return losses, accs

    def reward_paths(self, frames, shift=3):
        """frames uint8 [P, T, H, W, 3] -> P(expert) [P, T]."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim != 5 or frames.shape[2:] != (self.H, self.W, 3):
            raise ValueError(f"frames {frames.shape}, expected [P, T, {self.H}, {self.W}, 3]")
        P, T = frames.shape[:2]
        out = np.empty((P, T), np.float32)
        self._ck(self._lib.ctx_disc_reward_paths(self._h, frames.ctypes.data_as(_U8), P, T, int(shift), _fp(out)))
        return out

    @property
    def stream(self):
        """Integer hipStream_t of the handle: a FrameResizer made on it writes where the entries below read, in stream order."""
        return self._lib.ctx_disc_stream(self._h)

    def sync(self):
        self._ck(self._lib.ctx_disc_sync(self._h))

    def data_begin(self, N, T, classes, domains=None):
        """Sizes the resident data set for uint8 [N, T, H, W, 3] and uploads the per-trajectory targets like data_upload; returns the
        integer DEVICE address of the tensor, to be filled on `stream` (FrameResizer.resize_u8_dev(dst=address + offset)) before the
        next train_epoch."""
        N, T = int(N), int(T)
        cls = np.ascontiguousarray(classes, np.float32).reshape(N, 2)
        dom = None if domains is None else np.ascontiguousarray(domains, np.float32).reshape(N, 2)
        d = ctypes.c_void_p()
        self._ck(self._lib.ctx_disc_data_begin(self._h, N, T, _fp(cls), None if dom is None else _fp(dom), ctypes.byref(d)))
        return int(d.value)

    def reward_paths_dev(self, d_frames, P, T, shift=3):
        """reward_paths on DEVICE uint8 frames [P, T, H, W, 3] (integer address, any byte alignment, written on `stream` or before a
        sync) -> P(expert) [P, T]; same bits as reward_paths on the same bytes."""
        out = np.empty((int(P), int(T)), np.float32)
        self._ck(self._lib.ctx_disc_reward_paths_dev(self._h, ctypes.c_void_p(d_frames), int(P), int(T), int(shift), _fp(out)))
        return out


class DomainConfusionVelocityDiscriminator(_Discriminator):
    """discriminator.py:357-548 (mode 'tpil').  data_batch = [frames t, frames min(t+3, T-1)], targets_batch = dict(classes, domains)."""
    variant = CTX_DISC_TPIL

    def __init__(self, input_dim, output_dim_class=2, output_dim_dom=2, max_batch=32, device=0, seed=0):
        if output_dim_class != 2 or output_dim_dom != 2:
            raise ValueError("the heads are 2-way (cyberpunk_aws.py builds them with 2 and 2)")
        super().__init__(input_dim, max_batch=max_batch, device=device, seed=seed)

    def train(self, data_batch, targets_batch):
        return self._train(data_batch, targets_batch["classes"], targets_batch["domains"])

    def get_lab_accuracy(self, data, class_labels):
        return self._accuracy(data, class_labels)


class ConvDiscriminator(_Discriminator):
    """discriminator.py:122-207 (mode 'gail').  data_batch = [frames, time column], targets_batch = one-hot classes."""
    variant = CTX_DISC_GAIL

    def train(self, data_batch, targets_batch):
        return self._train(data_batch, targets_batch, None)

    def get_lab_accuracy(self, data, class_labels):
        return self._accuracy(data, class_labels)


def shuffled_order(n_traj, T):
    """shuffle_to_training_data's order (cyberpunk_trainer.py:165-166): the single np.random.permutation over (trajectory, t) rows.
    Row i of the reference's matrices is trajectory order[i] // T at time order[i] % T."""
    return np.random.permutation(int(n_traj) * int(T)).astype(np.int32)


def reward_pairs(n, shift=3):
    """cyberpunk_rollout (cyberpunk_trainer.py:231-235): a path of n frames is scored on the pairs (t, min(t + 3, n - 1))."""
    t = np.arange(int(n))
    return t, np.minimum(t + int(shift), int(n) - 1)


class ThirdPersonCost:
    """The cost side of CyberPunkTrainer.take_iteration (cyberpunk_trainer.py:100-116) and of its GAIL twin, on the device:
    set_data uploads the iteration's trajectories once and draws the shuffle as an index array, train_cost runs the epochs without
    materialising the shuffled matrices, path_rewards scores policy paths many per call."""
    shift = 3

    # how render-size frames reach the device: "block" = contiguous runs of frames, gathered on the host where a chunk spans several
    # arrays, one upload per chunk; "list" = one upload per frame from where it lies.  Measured (profiles/render_size_rewards.txt,
    # DESIGN.md section 10): the list form is 0.05-0.8 ms slower at 25 and at 250 frames, so the hook gathers.
    upload = "block"

    def __init__(self, disc, batch_size=32, logger=None, render_size=None, resize_chunk=256, resizer=None):
        """render_size=(Hr, Wr): set_data's trajectories and the paths' im_observations hold the frames as RENDERED, uint8
        [.., Hr, Wr, 3]; they are resized to the discriminator's size on the device (resize.FrameResizer on the discriminator's
        stream, resize_chunk frames per pass) and never come back: set_data resizes straight into the resident tensor, path_rewards
        into the buffer the first conv reads.  Results equal, bit for bit, those of the same object without render_size fed the
        frames resized on the host.  Float frames are refused (imresize rescales floats by their range, which is not what the rollout
        does).  resizer: an object with resize(frames) (and resize_u8_dev for the device chain) used instead of a FrameResizer; a
        discriminator without the device entries gets resizer.resize() followed by the host entry."""
        self.disc, self.batch_size, self.logger = disc, int(batch_size), logger
        self.gail = disc.variant == CTX_DISC_GAIL
        self.order = None
        self.log = []
        # render_size -> the discriminator's frame size, on the discriminator's stream, resize_chunk frames per pass
        self._render = RenderFrames(render_size, lambda: ((disc.H, disc.W), self.resize_chunk, getattr(disc, "device", 0), disc.stream),
                                    resizer)
        self.render_size = self._render.size
        self.resize_chunk = int(resize_chunk)
        if self.render_size is not None and self.resize_chunk < 1:
            raise ValueError(f"resize_chunk must be >= 1, got {resize_chunk}")

    _rs = property(lambda self: self._render.rs)                 # the resizer in use: the injected one, else a FrameResizer

    @staticmethod
    def _per_traj(a, what):
        a = np.asarray(a)
        if a.ndim == 3:
            if not (a == a[:, :1]).all():
                raise ValueError(f"{what} differ within a trajectory")
            a = a[:, 0]
        return a

    # ------------------------------------------------------------------ frames as rendered
    def _on_device(self):
        return self._render.on_device(self.disc, "reward_paths_dev", "data_begin")

    def _chunks_of(self, runs):
        """runs: arrays [m_i, Hr, Wr, 3] laid end to end -> per chunk of resize_chunk frames (chunks cross the arrays' boundaries)
        (first frame index, the chunk as one contiguous array or, in the list form, as a list of frames)."""
        total = sum(len(r) for r in runs)
        starts = np.cumsum([0] + [len(r) for r in runs])
        for i0 in range(0, total, self.resize_chunk):
            i1 = min(total, i0 + self.resize_chunk)
            parts = [r[max(i0 - s0, 0):i1 - s0] for r, s0 in zip(runs, starts[:-1]) if s0 < i1 and s0 + len(r) > i0]
            if self.upload == "list":
                yield i0, [f for part in parts for f in part]
            else:
                yield i0, (parts[0] if len(parts) == 1 else np.concatenate(parts))

    def _set_data_render(self, sets, cls, dom):
        datas = [self._render.check(np.asarray(s["data"]), 5, "a set's data") for s in sets]
        T = datas[0].shape[1]
        if any(d.shape[1] != T for d in datas):
            raise ValueError("every set must hold trajectories of the same length")
        N = sum(d.shape[0] for d in datas)
        if N * T == 0:
            raise ValueError("no frames")
        rs = self._render.resizer()
        runs = [d.reshape((-1,) + d.shape[2:]) for d in datas]
        if self._on_device():
            base, fbytes = self.disc.data_begin(N, T, cls, dom), self.disc.H * self.disc.W * 3
            # No sync happens between the chunks, and the resizer keeps only the latest call's frames (it waits only for copies it
            # made itself).  A chunk that spans arrays is an np.concatenate made HERE, which the resizer takes for the caller's: this
            # list is all that keeps those blocks, and the slices, alive until the uploads that read them are over (the sync below).
            held = []
            for i0, chunk in self._chunks_of(runs):
                held.append(chunk)
                rs.resize_u8_dev(chunk, dst=base + i0 * fbytes)
            rs.sync()                                             # the tensor is complete (and the frames released) before train_cost
        else:
            small = rs.resize(np.concatenate(runs))
            self.disc.data_upload(small.reshape((N, T) + small.shape[1:]), cls, dom)
        return N, T

    def set_data(self, expert, on_policy, expert_fail=None):
        """Each argument: dict(data [n, T, H, W, 3], classes [n, T, 2] or [n, 2], domains likewise) as collect_trajs_for_cost returns
        them; stacked in the reference's order (expert, on-policy, expert-fail; GAIL has no third set).  With render_size: data
        [n, T, Hr, Wr, 3] uint8 as rendered, resized resize_chunk frames at a time (chunks cross trajectory and set boundaries)
        straight into the resident tensor; the same single np.random.permutation is drawn."""
        sets = [s for s in (expert, on_policy, expert_fail) if s is not None]

        def targets():
            cls = np.concatenate([self._per_traj(s["classes"], "classes") for s in sets])
            return cls, None if self.gail else np.concatenate([self._per_traj(s["domains"], "domains") for s in sets])
        if self.render_size is not None:
            self.n_traj, self.T = self._set_data_render(sets, *targets())
        else:
            data = np.concatenate([np.asarray(s["data"]) for s in sets])
            if data.dtype != np.uint8:
                if (data != np.rint(data)).any() or data.min() < 0 or data.max() > 255:
                    raise ValueError("the resident data set holds uint8 frames: pass pixel values 0..255")
                data = data.astype(np.uint8)
            self.disc.data_upload(data, *targets())
            self.n_traj, self.T = data.shape[:2]
        self.order = shuffled_order(self.n_traj, self.T)
        return self.order

    def train_cost(self, n_epochs):
        """cyberpunk_trainer.py:140-159: n_epochs passes over the same order; per epoch the float64 np.mean of the batch losses and
        accuracies (GAIL: losses only), logged as GanLoss<i> / GanAcc<i>."""
        if self.order is None:
            raise RuntimeError("set_data first")
        out = []
        for it in range(int(n_epochs)):
            losses, accs = self.disc.train_epoch(self.order, self.batch_size, self.shift, with_accuracy=not self.gail)
            rec = {"GanLoss": np.mean(np.array(losses)), "GanAcc": None if accs is None else np.mean(np.array(accs))}
            if self.logger is not None:
                self.logger.record_tabular("GanLoss" + str(it), rec["GanLoss"])
                if accs is not None:
                    self.logger.record_tabular("GanAcc" + str(it), rec["GanAcc"])
            out.append(rec)
        self.log.extend(out)
        return out

    def path_rewards(self, paths):
        """path['rewards'] = P(expert) of the path's frames (path['im_observations'] [n, H, W, 3]).  A rollout that ends early has fewer
        frames than the horizon: paths are grouped by length, one device call per length, the +3 partner clamped to each path's own
        last frame.  With render_size: im_observations [n, Hr, Wr, 3] uint8 as rendered; per length as many whole paths per call as
        fit resize_chunk frames are resized on the device and scored where they lie.  A path longer than resize_chunk raises
        resize_chunk to that path's length, once and for good (the resizer is remade at that size)."""
        by_len = {}
        for i, p in enumerate(paths):
            by_len.setdefault(len(p["im_observations"]), []).append(i)
        if self.render_size is not None:
            score = self._render_scorer(paths, by_len)
        else:
            def score(grp, n):
                frames = np.stack([np.asarray(paths[i]["im_observations"]) for i in grp])
                if frames.dtype != np.uint8:
                    frames = np.rint(frames).astype(np.uint8)
                return self.disc.reward_paths(frames, self.shift)
        for n, idx in by_len.items():
            if n == 0:
                for i in idx:
                    paths[i]["rewards"] = np.zeros(0, np.float32)
                continue
            per = len(idx) if self.render_size is None else max(1, self.resize_chunk // n)
            for k0 in range(0, len(idx), per):
                grp = idx[k0:k0 + per]
                r = score(grp, n)
                for k, i in enumerate(grp):
                    paths[i]["rewards"] = r[k].copy()
        return paths

    def _render_scorer(self, paths, by_len):
        """score(grp, n) -> r[len(grp), n] for paths of n frames as rendered, checked here: an array [n, Hr, Wr, 3] stays one block,
        a list of frames stays a list, where they lie."""
        obs = {i: self._render.check(paths[i]["im_observations"], 4, "im_observations") for n, idx in by_len.items() if n for i in idx}
        longest = max([n for n in by_len], default=0)
        if longest > self.resize_chunk:                            # one path must fit one pass
            self.resize_chunk = longest
            self._render.drop()
        rs = self._render.resizer() if obs else None
        if obs and self._on_device():
            def score(grp, n):                                     # returns after the stream is drained
                src = gather([obs[i] for i in grp], self.upload == "list")
                return self.disc.reward_paths_dev(rs.resize_u8_dev(src), len(grp), n, self.shift)
        else:
            def score(grp, n):
                small = rs.resize(gather([obs[i] for i in grp]))
                return self.disc.reward_paths(small.reshape((len(grp), n) + small.shape[1:]), self.shift)
        return score
