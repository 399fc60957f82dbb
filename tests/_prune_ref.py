"""A plain statement of which backward launch groups a mask of trainable tensors needs, for tests/test_prune_ref.py and
tests/test_gpu_mask_sweep.py.  It is written from the models' dataflow, not from csrc/ctx_engine.cpp's plan_mask: a group is a node that
reads gradient signals and writes gradient signals or parameter gradients, and a mask needs a group iff a trainable tensor's gradient
is reachable from it.

Group names are ctx_profile_step's: "<scope>/<layer> dw|db|dx", "conv/hz_lin lrelu'", "losses".

ContextSkipNew, from the loss back:
  losses                 writes d out (= d of d_h4's output) and the simloss seed
  deconv/d_hk  dw, db    read d (d_hk output);  dx also writes d (d_h(k-1) output) -- k = 1: d dz, d_h0_lin's output -- and d (ctx skip h_(4-k))
  deconv/d_h0_lin        reads d dz (+ the seed); dx writes d trans_z and d tgt_z
  translate/trans_z      reads d trans_z; dx writes d trans_h0
  translate/trans_h0     reads d trans_h0; dx writes d src_z and d ctx_z
  conv/hz_lin lrelu'     reads d tgt_z and d src_z (`conv` encodes [tgt | src] in one batch), writes d (conv/hz_lin output)
  <enc>/<layer l>        layers h0_conv .. h3_conv, h4_lin, hz_lin; dw, db read d (layer l output); dx (l >= 1) also reads, in
                         `conv_context`, both passes' d (ctx skip h_(l-1)) and writes d (layer l-1 output).  conv_context/hz_lin's
                         output gradient is d ctx_z.

The table-driven engine (ContextAEReal, ContextAEInception2) prunes less ("Out of scope"): needed_table()."""
from collections import OrderedDict

ENC_LAYERS = ["h0_conv", "h1_conv", "h2_conv", "h3_conv", "h4_lin", "hz_lin"]
FC_MIDDLE = ["translate/trans_h0", "translate/trans_z", "deconv/d_h0_lin"]
LOSSES, LRELU = "losses", "conv/hz_lin lrelu'"
RCHAIN = ("d_h0_lin .. h4_lin dx", "h4_lin .. d_h0_lin dw db")
# on the direct 3-channel route the first encoder layer's bias gradient leaves the filter-gradient launch: no `db` group of its own
FOLDED = {"conv/h0_conv db": "conv/h0_conv dw", "conv_context/h0_conv db": "conv_context/h0_conv dw"}


def tensor_pair(layer):
    """(filter / Matrix, bias) tensor names of a layer"""
    return (layer + "/w", layer + "/biases") if layer.endswith("_conv") or layer[-1] in "1234" else (layer + "/Matrix", layer + "/bias")


def layers(scopes=("conv_context", "conv")):
    out = [sc + "/" + l for sc in scopes for l in ENC_LAYERS]
    return out + FC_MIDDLE + ["deconv/d_h%d" % k for k in (1, 2, 3, 4)]


def tensor_names(scopes=("conv_context", "conv")):
    """every tensor of a model with these encoder scopes, in arena order (38 names, or 26 for ContextAEReal's single `conv`)"""
    return [t for l in layers(scopes) for t in tensor_pair(l)]


def skipnew_graph():
    """group -> (signals read, signals written, parameter gradient written or None)"""
    G = OrderedDict()
    G[LOSSES] = ((), ("d:deconv/d_h4", "d:seed"), None)

    def own(layer, sig):
        w, b = tensor_pair(layer)
        G[layer + " dw"] = ((sig,), (), w)
        G[layer + " db"] = ((sig,), (), b)
    for k in (4, 3, 2, 1):
        L, sig = "deconv/d_h%d" % k, "d:deconv/d_h%d" % k
        own(L, sig)
        G[L + " dx"] = ((sig,), ("d:deconv/d_h%d" % (k - 1) if k > 1 else "d:dz", "d:skip%d" % (4 - k)), None)
    own("deconv/d_h0_lin", "d:dz")
    G["deconv/d_h0_lin dx"] = (("d:dz", "d:seed"), ("d:trans_z", "d:tgt_z"), None)
    own("translate/trans_z", "d:trans_z")
    G["translate/trans_z dx"] = (("d:trans_z",), ("d:trans_h0",), None)
    own("translate/trans_h0", "d:trans_h0")
    G["translate/trans_h0 dx"] = (("d:trans_h0",), ("d:src_z", "d:ctx_z"), None)
    G[LRELU] = (("d:tgt_z", "d:src_z"), ("d:conv/hz_lin",), None)
    for sc in ("conv", "conv_context"):
        for l in range(5, -1, -1):
            L = sc + "/" + ENC_LAYERS[l]
            sig = "d:ctx_z" if L == "conv_context/hz_lin" else "d:" + L
            own(L, sig)
            if l:
                reads = (sig,) + (("d:skip%d" % (l - 1),) if sc == "conv_context" and l - 1 <= 3 else ())
                G[L + " dx"] = (reads, ("d:" + sc + "/" + ENC_LAYERS[l - 1],), None)
    return G


_G = skipnew_graph()
SKIPNEW_GROUPS = list(_G)


def needed(trainable):
    """ContextSkipNew: the set of backward groups from which the gradient of a tensor in `trainable` is reachable (plus `losses`,
    which also forms the step's scalars)"""
    trainable = set(trainable)
    unknown = trainable - set(tensor_names())
    assert not unknown, f"no such tensor: {sorted(unknown)}"
    need = {g for g, (_, _, par) in _G.items() if par in trainable} | {LOSSES}
    while True:
        wanted = {s for g in need for s in _G[g][0]}                 # signals a needed group reads
        more = {g for g, (_, writes, _) in _G.items() if wanted & set(writes)} - need
        if not more:
            return need
        need |= more


def classify_table(name):
    """kind of a backward group of the table-driven engine: 'always', or ('decoder', layer) / ('fc', tensor).  Unknown: KeyError."""
    if name in (LOSSES, LRELU) + RCHAIN or name.endswith(" dx"):
        if name.endswith(" dx") and name not in RCHAIN and name[:-3] not in layers():
            raise KeyError(name)
        return "always"
    layer, _, kind = name.rpartition(" ")
    if kind not in ("dw", "db") or layer not in layers():
        raise KeyError(name)
    if layer.startswith(("conv/", "conv_context/")):
        return "always"
    if layer in FC_MIDDLE:
        return ("fc", tensor_pair(layer)[kind == "db"])
    return ("decoder", layer)


def needed_table(trainable, full_groups):
    """The table-driven engine: of the unmasked backward's groups, encoder groups and every input gradient always run (both
    `rchain` groups with them), a decoder layer's dw / db iff one of its two tensors trains, an FC-middle dw / db by its own tensor."""
    trainable = set(trainable)
    need = set()
    for g in full_groups:
        kind = classify_table(g)
        if kind == "always" or (kind[0] == "fc" and kind[1] in trainable) or (kind[0] == "decoder" and set(tensor_pair(kind[1])) & trainable):
            need.add(g)
    return need


def unclassified(full_groups, table_driven):
    """names of an unmasked backward the model does not know: a new launch group must be given its place here first"""
    bad = []
    for g in full_groups:
        if table_driven:
            try:
                classify_table(g)
            except KeyError:
                bad.append(g)
        elif g not in _G:
            bad.append(g)
    return bad


def sibling(group):
    """the other of a layer's dw / db pair (co-scheduled in conv-type layers), or None"""
    layer, _, kind = group.rpartition(" ")
    return layer + (" db" if kind == "dw" else " dw") if kind in ("dw", "db") and layer in layers() else None


def check_groups(got, need, full):
    """`got` (the device's backward groups under a mask) against `need`: contains what of `need` the unmasked backward `full` has --
    a folded bias gradient through the launch it is folded into --, holds nothing beyond `need` and the siblings of needed groups, in
    the unmasked order.  Returns the sibling allowances used."""
    got_s, full_s = set(got), set(full)
    want = {g if g in full_s else FOLDED.get(g) for g in need}
    assert None not in want, f"needed groups the unmasked backward does not have: {sorted(g for g in need if g not in full_s and g not in FOLDED)}"
    assert want <= got_s, f"needed and not run: {sorted(want - got_s)}"
    extra = got_s - want
    allowed = {sibling(g) for g in want}
    assert extra <= allowed, f"run and not needed: {sorted(extra - allowed)}"
    assert got_s <= full_s and [g for g in full if g in got_s] == list(got), "not the unmasked order"
    return sorted(extra)
