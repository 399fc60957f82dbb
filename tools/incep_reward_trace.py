"""Kernel shares of a `rocprofv3 --kernel-trace --stats` run of tools/bench_inception_reward.py: each stats / cost kernel launch
against the front-end forward it reads (the kernels since the forward's pad_channels launch).
    python tools/incep_reward_trace.py <rocprofv3 results .db>"""
import sqlite3, sys, collections
db = sqlite3.connect(sys.argv[1])
rows = list(db.execute("select name, start, end, duration, grid_x from kernels order by start"))
def short(n):
    for k in ("incep_cost_kernel", "stats_accum_kernel", "stats_finish_kernel", "avgpool_valid_kernel", "pad_channels_kernel"):
        if k in n:
            return k + ("<4>" if "<4>" in n else "<1>" if "<1>" in n else "")
    return "front end (other kernels)"
layer = "Mixed_7c"
fw = 0.0; cur_fw_kernels = 0
seg = collections.defaultdict(lambda: collections.defaultdict(list))   # layer -> kind -> [(kernel ns, forward ns)]
tot = collections.defaultdict(lambda: collections.defaultdict(float))
for name, s, e, d, gx in rows:
    k = short(name)
    if k == "avgpool_valid_kernel":
        layer = "PreLogits"
    if k == "pad_channels_kernel":
        fw = 0.0
    tot[layer][k] += d
    if k.startswith("incep_cost") or k.startswith("stats_accum"):
        seg[layer][k.split("<")[0]].append((d, fw))
    elif k != "stats_finish_kernel":
        fw += d
for L in ("Mixed_7c", "PreLogits"):
    print(f"== layer {L}: kernel totals over the run (ms)")
    for k, v in sorted(tot[L].items(), key=lambda kv: -kv[1]):
        print(f"   {k:32s} {v / 1e6:9.3f}")
    for k, lst in seg[L].items():
        kd = sum(a for a, _ in lst); fd = sum(b for _, b in lst)
        print(f"   {k}: {len(lst)} launches, {kd / len(lst) / 1e3:.1f} us each; the forwards they read {fd / len(lst) / 1e6:.2f} ms each "
              f"-> {100 * kd / fd:.2f} % of the front end's time on the same frames")
