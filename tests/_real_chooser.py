"""Python restatement of the tile choice of dconv_launch (csrc/dconv.hip) for exact f32 on a 256-CU device with 160 KiB of LDS per CU, and
the four-class launches of ContextAEReal that reach it.  Test infrastructure only: tests/test_real_trace_lines.py holds it to lines traced
on an MI355X and reads from it which (MI, NB) and which partial tiles the chooser can pick on legal shapes up to 64x192 -- the claim behind
INVENTORY and UNREACHED of tests/test_gpu_real_routes.py.  In exact f32 the one-class launches with 16 or 32 input channels go to
dconv_launch2 and never reach this chooser."""
LDS_TOTAL = 160 * 1024
LDS_BUDGET = LDS_TOTAL - 4096
DC_NW, DC_THREADS, DC_PF, DC_PF_SMALL = 8, 512, 12, 4                   # csrc/dconv.h
TAPS4 = (9, 6, 6, 4)                                                    # the parity classes of a stride-2 transposed conv (dconv_convt2)
# (layer, input channels, output columns, what divides H and W to its grid)
LAYERS = (("d_h1 fwd", 16, 16, 4), ("d_h3 fwd", 32, 32, 2), ("h3 dx", 8, 16, 4), ("h1 dx", 16, 32, 2))


def cik_of(ci):
    return 4 if ci == 3 else 8 if ci <= 8 else 16 if ci <= 16 else 32 if ci <= 32 else 64


def dc_cip(cik, S):
    return 4 if cik == 4 else (8 if S == 1 else 12) if cik == 8 else cik + (8 if S == 1 else 4)


def fwd_cfg_ok(mi, nb):
    return mi <= 4 if nb == 1 else mi <= 3 if nb == 2 else mi <= 2 if nb == 4 else False


def choose(CI, N, S, span, taps, hlog, wlog):
    """dict(TH, TW, MI, NB, occ, slices, tiles_y, tiles_x) as dconv_launch picks them."""
    CIK = cik_of(CI)
    CIP = dc_cip(CIK, S)
    NBT = (N + 15) // 16
    NBT = 1 if NBT <= 1 else 2 if NBT <= 2 else 4 if NBT <= 4 else 8
    TPC, CPT = (1, CIK // 16) if CIK >= 16 else (16 // CIK, 1)
    nslots = nchunks = 0
    for t in taps:
        ntp = (t + TPC - 1) // TPC * TPC
        nslots += ntp
        nchunks += ntp // TPC * CPT
    per_pixel = 3 if CIK == 4 else CIK // 4
    best, pick = -1.0, None
    nb = min(NBT, 4)
    while nb >= 1:
        wall = nslots * CIK * nb * 16 * 4 + (nslots * CIK // 16 + 1) * 16
        tw = 16
        while tw <= 64 and tw <= (wlog + 15) // 16 * 16:
            mi = 1
            while mi <= 4 and fwd_cfg_ok(mi, nb):
                for th in range(1, 33):
                    nrb = th * (tw // 16)
                    if nrb > DC_NW * mi:
                        break
                    if mi > 1 and nrb <= DC_NW * (mi - 1):
                        continue
                    ih, iw = S * (th - 1) + span, S * (tw - 1) + span
                    tile = ((ih * iw * CIP + 3) & ~3) * 4
                    if tile + wall > LDS_BUDGET or ih * iw * per_pixel > DC_THREADS * DC_PF:
                        break
                    busiest = max(1, (nrb + 3) // 4)
                    occ = 2 if (nb == min(NBT, 4) and 2 * (tile + wall) + 1024 <= LDS_TOTAL and mi * nb <= 2 and
                                ih * iw * per_pixel <= DC_THREADS * DC_PF_SMALL) else 1
                    ty, tx = (hlog + th - 1) // th, (wlog + tw - 1) // tw
                    rows = hlog * wlog / (ty * tx)
                    compute = busiest * nb * nchunks * 4 * 32.0
                    T = max(compute, tile / 16.0) + (tile / 79.0 + 3000.0 + 40.0 * mi * nb * len(taps)) / occ
                    score = rows / (T * (NBT // nb))
                    if score > best:
                        best, pick = score, dict(TH=th, TW=tw, MI=mi, NB=nb, occ=occ, slices=-(-N // (nb * 16)), tiles_y=ty, tiles_x=tx)
                mi += 1
            tw *= 2
        nb //= 2
    return pick


def picks(heights=range(4, 65, 4), widths=(64, 128, 192)):
    """{(MI, NB, occ, slices, partial-y, partial-x)} over the four-class launches of every legal shape."""
    out = set()
    for W in widths:
        for H in heights:
            for _, CI, N, d in LAYERS:
                c = choose(CI, N, 1, 3, TAPS4, H // d, W // d)
                out.add((c["MI"], c["NB"], c["occ"], c["slices"], int((H // d) % c["TH"] != 0), int((W // d) % c["TW"] != 0)))
    return out
