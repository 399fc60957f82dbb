"""CPU statement of the two baseline discriminators (torch autograd in float64 / float32 + a plain numpy forward): what the GPU tests
of ctx_disc_* compare against.  A restatement, line by line, of sandbox/bradly/third_person/discriminators/discriminator.py (cited as
D:<lines>), flip_gradients.py and the loops of algos/cyberpunk_trainer.py (T:<lines>) / cyberpunk_trainer_gail.py (G:<lines>).
Nothing here reads the reference tree.

Layouts are the reference's: frames NHWC with raw pixel values 0..255, filters HWIO, FC weights [in, out]."""
import numpy as np
import torch
import torch.nn.functional as F

TPIL, GAIL = 0, 1
NF, HID = 5, 128            # D:150 / D:394 num_filters = [5, 5]; layer_size = 128
DOM_W = 0.2                 # D:471 flip_gradient(..., l=0.2) and D:483 loss = class_loss + 0.2 * dom_loss
FC_RELU = {TPIL: ("f", "hc1", "hc2", "hd1", "hd2"), GAIL: ("hc1",)}


def pooled(n):
    return -(-n // 2)       # 'SAME' pooling with stride 2: ceil(n / 2)   (D:54-55)


def param_shapes(variant, H, W):
    """name -> shape in the reference's variable creation order (D:159-170, D:408-419 / :445-446, get_mlp_layers D:57-75)."""
    h2, w2 = pooled(H), pooled(W)
    s = [("wc1", (3, 3, 3, NF)), ("wc2", (3, 3, NF, NF)), ("bc1", (NF,)), ("bc2", (NF,))]
    if variant == TPIL:
        n = pooled(h2) * pooled(w2) * NF
        s += [("w_feats_one", (n, HID)), ("b_feats_one", (HID,))]
        for pre, k0 in (("targets", 2 * HID), ("dom", HID)):
            dims = [k0, HID, HID, 2]
            for k in range(3):
                s += [(f"w_{pre}{k}", (dims[k], dims[k + 1])), (f"b_{pre}{k}", (dims[k + 1],))]
    else:
        if H % 2 or W % 2:
            raise ValueError("ConvDiscriminator: int(W*H*5/4) is the pooled size only for even H and W (D:156)")
        s += [("w_0", (h2 * w2 * NF + 1, HID)), ("b_0", (HID,)), ("w_1", (HID, 2)), ("b_1", (2,))]
    return s


def init_params(variant, H, W, seed):
    """D:41-47 (FC: N(0, 0.01), biases 0) and D:77-84 (filters: uniform +- 4 sqrt(6 / (fan_in + fan_out)), the fans taken from the HWIO
    shape as written: fan_in = prod(shape[1:]), fan_out = shape[0] * prod(shape[2:]) // 4)."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(variant, H, W):
        if len(shape) == 4:
            fan_in = np.prod(shape[1:])
            fan_out = shape[0] * np.prod(shape[2:]) // 4
            b = 4 * np.sqrt(6.0 / (fan_in + fan_out))
            P[name] = rng.uniform(-b, b, shape)
        elif len(shape) == 2:
            P[name] = rng.normal(0, 0.01, shape)
        else:
            P[name] = np.zeros(shape)
    return P


def flatten_params(P, dtype=np.float32):
    return np.concatenate([np.asarray(v, dtype).ravel() for v in P.values()])


def unflatten(flat, variant, H, W):
    out, o = {}, 0
    for name, shape in param_shapes(variant, H, W):
        n = int(np.prod(shape))
        out[name] = np.asarray(flat[o:o + n]).reshape(shape)
        o += n
    assert o == len(flat)
    return out


class _Flip(torch.autograd.Function):
    """flip_gradients.py: identity forward, gradient times -l backward."""

    @staticmethod
    def forward(ctx, x, l):
        ctx.l = l
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return -g * ctx.l, None


def _windows(y):
    """[N,C,H,W] -> [N,C,H2,W2,4]: the 2x2 SAME windows in row-major order, the missing row / column of an odd side = -inf."""
    H, W = y.shape[2:]
    y = F.pad(y, (0, W % 2, 0, H % 2), value=float("-inf"))
    N, C, Hp, Wp = y.shape
    return y.reshape(N, C, Hp // 2, 2, Wp // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Hp // 2, Wp // 2, 4)


def first_max(win, tol=0.0):
    """numpy [..., 4] -> index of the first maximum while scanning with a strict > (what the CPU kernels of TF and torch do).
    tol: a later element replaces the running maximum only if it exceeds it by more than tol * |maximum|.  The float64 statement
    records its own choice with tol = 1e-12: torch's float64 convolution sums in an order that depends on the position, so outputs
    that are EXACTLY tied in exact arithmetic (flat colour regions) come out a few ulp (1e-16) apart, and a tie must count as a tie
    -- both sides pick the first.  1e-12 is four orders above float64 rounding and five below float32's, so every choice that a
    float32 implementation can actually get differently is still seen."""
    best = win[..., 0].copy()
    idx = np.zeros(best.shape, np.int64)
    for p in range(1, 4):
        gt = win[..., p] > best + tol * np.abs(best)
        idx[gt] = p
        best = np.where(gt, win[..., p], best)
    return idx


def _conv_pool(x, w, b, rec, key, sel):
    """x NHWC -> NHWC: D:49-55, relu(conv3x3 SAME + b) then 2x2 SAME max pool.  sel (optional): the pool selections to USE instead of
    this precision's own, [N,H2,W2,C] codes winner + 4 * (maximum > 0) -- the value and the gradient then follow that choice."""
    pre = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1)
    win = _windows(pre)
    wn = win.detach().numpy()
    own_idx = first_max(np.maximum(wn, 0.0), 1e-12 if wn.dtype == np.float64 else 0.0)
    own_act = np.maximum(wn, 0.0).max(-1) > 0
    rec[key] = (own_idx + 4 * own_act).transpose(0, 2, 3, 1)
    if sel is None:
        y = F.relu(pre)
        H, W = y.shape[2:]
        out = F.max_pool2d(F.pad(y, (0, W % 2, 0, H % 2), value=float("-inf")), 2)
    else:
        code = torch.as_tensor(np.asarray(sel).astype(np.int64)).permute(0, 3, 1, 2)
        out = torch.gather(win, 4, (code & 3).unsqueeze(-1)).squeeze(-1) * ((code & 4) > 0).to(win.dtype)
    return out.permute(0, 2, 3, 1)


def _fc(x, w, b, rec, key, choices, relu=True):
    t = x @ w + b
    if not relu:
        return t
    rec[key] = (t.detach().numpy() > 0)
    if choices is not None and key in choices:
        return t * torch.as_tensor(np.asarray(choices[key]) > 0).to(t.dtype)
    return F.relu(t)


def _ce(logits, target):
    """D:486-488: reduce_mean(softmax_cross_entropy_with_logits) over the rows fed."""
    return (-(target * F.log_softmax(logits, 1)).sum(1)).mean()


def model(P, x1, x2t, cls, dom, variant, reversal=True, choices=None):
    """P: dict of torch tensors.  x1 [B,H,W,3]; x2t: TPIL second frames, GAIL time [B].  choices: ReLU masks / pool selections to take
    (the device's) instead of this precision's own.  Returns a dict with loss, class_loss, dom_loss, logits and rec (own choices)."""
    rec = {}
    ch = choices or {}
    if variant == TPIL:
        B = x1.shape[0]
        x = torch.cat([x1, x2t], 0)                                               # both images through the same trunk (D:421-449)
        h = _conv_pool(x, P["wc1"], P["bc1"], rec, "sel1", ch.get("sel1"))
        h = _conv_pool(h, P["wc2"], P["bc2"], rec, "sel2", ch.get("sel2"))
        f = _fc(h.reshape(h.shape[0], -1), P["w_feats_one"], P["b_feats_one"], rec, "f", choices)
        f1, f2 = f[:B], f[B:]
        t = torch.cat([f1, f2], 1)                                                # D:451
        t = _fc(t, P["w_targets0"], P["b_targets0"], rec, "hc1", choices)
        t = _fc(t, P["w_targets1"], P["b_targets1"], rec, "hc2", choices)
        lc = _fc(t, P["w_targets2"], P["b_targets2"], rec, None, None, relu=False)
        d = _Flip.apply(f1, DOM_W) if reversal else f1                            # D:471
        d = _fc(d, P["w_dom0"], P["b_dom0"], rec, "hd1", choices)
        d = _fc(d, P["w_dom1"], P["b_dom1"], rec, "hd2", choices)
        ld = _fc(d, P["w_dom2"], P["b_dom2"], rec, None, None, relu=False)
        class_loss = _ce(lc, cls) if cls is not None else None
        dom_loss = _ce(ld, dom) if dom is not None else None
        loss = class_loss + DOM_W * dom_loss if cls is not None and dom is not None else None     # D:483
    else:
        h = _conv_pool(x1, P["wc1"], P["bc1"], rec, "sel1", ch.get("sel1"))      # conv2 is commented out (D:177-181)
        t = torch.cat([h.reshape(h.shape[0], -1), x2t.reshape(-1, 1)], 1)         # D:183
        t = _fc(t, P["w_0"], P["b_0"], rec, "hc1", choices)
        lc = _fc(t, P["w_1"], P["b_1"], rec, None, None, relu=False)
        class_loss = _ce(lc, cls) if cls is not None else None
        dom_loss = None
        loss = class_loss
    return dict(loss=loss, class_loss=class_loss, dom_loss=dom_loss, logits=lc, rec=rec)


def run(Pn, x1, x2t, cls, dom, variant, dtype=torch.float64, reversal=True, choices=None, which="loss"):
    """numpy in, numpy out: loss, logits, probs, accuracy, gradients by name (zeros where a variable gets none), own choices."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in Pn.items()}
    tt = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    r = model(P, tt(x1), tt(x2t), tt(cls), tt(dom), variant, reversal, choices)
    out = dict(logits=r["logits"].detach().double().numpy(), rec=r["rec"])
    out["probs"] = F.softmax(r["logits"].detach(), 1).double().numpy()
    if cls is not None:
        out["loss"] = float(r["loss"].detach()) if r["loss"] is not None else None
        out["class_loss"] = float(r["class_loss"].detach())
        out["dom_loss"] = None if r["dom_loss"] is None else float(r["dom_loss"].detach())
        out["accuracy"] = accuracy(out["logits"], cls)
        if r[which] is not None:
            r[which].backward()
            out["grads"] = {k: (v.grad.double().numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return out


def accuracy(logits, cls):
    """D:465-467, :519-522: mean(argmax(class_target) == argmax(softmax(logits))); argmax takes the first index on ties."""
    return float(np.mean(np.argmax(np.asarray(cls), 1) == np.argmax(np.asarray(logits), 1)))


B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))     # TF keeps beta1 / beta2 (and their powers) as float32 values


def adam_tf(p, g, m, v, t, lr, b1=B1, b2=B2, eps=1e-8):
    """tf.train.AdamOptimizer in closed form (eps outside the bias correction); t = 1 for the first step.  Returns p, m, v."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def trajectory(Pn, batches, variant, lr, steps, dtype):
    """`steps` Adam steps cycling through `batches` [(x1, x2t, cls, dom)]: per-step losses and the final parameters, in `dtype`
    arithmetic throughout (np.float32 or np.float64)."""
    td = torch.float32 if dtype == np.float32 else torch.float64
    P = {k: np.asarray(v, dtype) for k, v in Pn.items()}
    M = {k: np.zeros_like(v) for k, v in P.items()}
    V = {k: np.zeros_like(v) for k, v in P.items()}
    losses = []
    for s in range(steps):
        x1, x2t, cls, dom = batches[s % len(batches)]
        r = run(P, x1, x2t, cls, dom, variant, td)
        losses.append(r["loss"])
        for k in P:
            g = r["grads"][k].astype(dtype)
            p, m, v = adam_tf(P[k], g, M[k], V[k], dtype(s + 1), dtype(lr), dtype(B1), dtype(B2), dtype(1e-8))
            P[k], M[k], V[k] = p.astype(dtype), m.astype(dtype), v.astype(dtype)
    return losses, P


# ---- the plain numpy forward (no torch): pins the torch statement ----------------------------------------------------------------
def _np_conv_pool(x, w, b):
    N, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    y = np.zeros((N, H, W, w.shape[3])) + b
    for ky in range(3):
        for kx in range(3):
            y = y + np.einsum("nhwc,cf->nhwf", xp[:, ky:ky + H, kx:kx + W, :], w[ky, kx])
    y = np.maximum(y, 0)
    y = np.pad(y, ((0, 0), (0, H % 2), (0, W % 2), (0, 0)), constant_values=-np.inf)
    return y.reshape(N, (H + 1) // 2, 2, (W + 1) // 2, 2, -1).max(axis=(2, 4))


def forward_np(P, x1, x2t, variant):
    """class logits in float64 numpy"""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    relu = lambda a: np.maximum(a, 0)
    if variant == TPIL:
        B = len(x1)
        h = _np_conv_pool(_np_conv_pool(np.concatenate([x1, x2t]).astype(np.float64), P["wc1"], P["bc1"]), P["wc2"], P["bc2"])
        f = relu(h.reshape(len(h), -1) @ P["w_feats_one"] + P["b_feats_one"])
        t = np.concatenate([f[:B], f[B:]], 1)
        for k in range(3):
            t = t @ P[f"w_targets{k}"] + P[f"b_targets{k}"]
            if k < 2:
                t = relu(t)
        return t
    h = _np_conv_pool(np.asarray(x1, np.float64), P["wc1"], P["bc1"])
    t = np.concatenate([h.reshape(len(h), -1), np.asarray(x2t, np.float64).reshape(-1, 1)], 1)
    return relu(t @ P["w_0"] + P["b_0"]) @ P["w_1"] + P["b_1"]


# ---- the loops -------------------------------------------------------------------------------------------------------------------
def shuffle_rows(n_traj, T, shift=3):
    """T:161-183 as index arithmetic: ONE np.random.permutation over the (trajectory, t) grid; row i = (trajectory, t, min(t+shift, T-1))."""
    perm = np.random.permutation(n_traj * T)
    traj, t = perm // T, perm % T
    return traj, t, np.minimum(t + shift, T - 1)


def reward_pairs(n, shift=3):
    """T:231-237: the pairs (t, min(t + 3, n - 1)) of a path of n frames."""
    t = np.arange(n)
    return t, np.minimum(t + shift, n - 1)


def count_flips(own, dev, variant):
    """(differing choices, all choices) between this statement's own ReLU / pool decisions and the device's.  A pool window counts once:
    different if the live flags differ, or both live and the winners differ."""
    bad = tot = 0
    for k in ("sel1", "sel2"):
        if k in own and k in dev:
            a, b = np.asarray(own[k]).astype(np.int64), np.asarray(dev[k]).astype(np.int64)
            la, lb = (a & 4) > 0, (b & 4) > 0
            bad += int(np.sum((la != lb) | (la & lb & ((a & 3) != (b & 3)))))
            tot += a.size
    for k in FC_RELU[variant]:
        if k in own and k in dev:
            bad += int(np.sum(np.asarray(own[k]) != (np.asarray(dev[k]) > 0)))
            tot += np.asarray(own[k]).size
    return bad, tot
