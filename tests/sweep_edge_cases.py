"""The CAQR pair sweep at its column-window, tile and schedule edges: a case table made BY RULE (test infrastructure: nothing here
is on the product path, nothing here touches a GPU).

`sweep_trace(batch, m, n, t_list, env, tile_rows)` restates run_caqr (enlsip_gn.hip), plan_geometry (gn_plan.hpp) and the block
kernels' own branches (gn_kernels_update_v4.hpp: v4_setup, k_caqr_update_v4, k_caqr_update_v4_pair, launch_update_v4) as a pure
function: the list of level-0 window-update launches of a solve whose constraint matrices have full rank, each with its window, its
grid and the form every column block takes.  The constants are parsed from the sources, not copied.  `edges(trace)` names the edge
values a trace contains; `cases()` builds, family by family (A far-window width, B rows, C tile octets, D look-ahead sub-windows,
E mixed widths under forced pairs), the smallest shapes whose traces together contain every name of `required_edges()`;
tests/test_sweep_edge_cases_host.py certifies that cover, its minimality (no case can be removed) and the reference floors on the
CPU, tests/test_gpu_sweep_edges.py runs the table on the device and holds the reported route against the trace."""
from __future__ import annotations

import re

import dispatch_grid as dg

PB = dg.PB
_UPD = (dg.CSRC / "gn_kernels_update_v4.hpp").read_text()
_HIP = (dg.CSRC / "enlsip_gn.hip").read_text()
_PLAN = (dg.CSRC / "gn_plan.hpp").read_text()


def _find(txt: str, pattern: str, what: str) -> tuple:
    mt = re.search(pattern, txt)
    assert mt, what
    return tuple(int(g) for g in mt.groups())


CW, = _find(_UPD, r"#define ENLSIP_V4_CW (\d+)", "ENLSIP_V4_CW")                       # columns per workgroup of the block kernels
XMAP_MAX_BATCH, XMAP_MIN_TILES = _find(_HIP, r"xmap_tiles = .*P\.batch <= (\d+) && groups >= (\d+) && !mixed", "xmap_tiles")
NEAR_PAIR, = _find(_HIP, r"two_streams\(nfar, (\d+) \* PB, far_update\)", "near width of the paired look-ahead")     # in panels
NEAR_PLAIN, = 1,
assert re.search(r"two_streams\(ntrail, PB, ", _HIP), "near width of the plain look-ahead"
PAIR_MIN_WGS, = _find(_PLAN, r"PLAN_PAIR_MIN_WGS = (\d+)", "PLAN_PAIR_MIN_WGS")
LA_MAX_BATCH, LA_MIN_WGS = _find(_HIP, r"\(\(P\.batch <= (\d+) && far_wgs0 >= (\d+)\) \|\| h->lookahead_forced\)", "look-ahead by size")
assert CW == PB == 32, "the block forms below are written for 32-column blocks of 32-column panels"

SIZE_CAP = 2_500_000          # m * n of a case
BATCH_CAP = 9


def _rup(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _levels(m: int, n: int, kA: int, batch: int, tile_rows: int, env: dict) -> tuple:
    """plan_geometry: (pair, RPL, per panel (tiles, valid units of the last tile, tree levels))."""
    rpl = (256 if m <= 256 else tile_rows) // 64
    F = 2 * rpl
    kpmax = min(m, n)
    npan_max = (kpmax + PB - 1) // PB
    far_wgs = batch * ((max(m, 1) + 64 * rpl - 1) // (64 * rpl)) * ((max(n - kA, 1) + 31) // 32)
    pair_env = env.get("ENLSIP_GN_PAIR", "")
    pair = pair_env != "0" and npan_max >= 3 and (far_wgs >= PAIR_MIN_WGS or pair_env in ("1", "2"))
    mpad = _rup(max(m, 1), 32)
    panels = []
    for k in range(npan_max):
        second = pair and (k & 1)
        anchor = 32 * (k - (1 if second else 0))
        nb0 = (mpad - anchor) // 32
        tiles = (nb0 + F - 1) // F
        last_units = nb0 - (tiles - 1) * F
        tree = 0
        if tiles > 1:
            if second:
                nblocks1 = (tiles - (1 if last_units == 1 else 0)) + (tiles - 1)
                nb = (nblocks1 + F - 1) // F
                tree = 1
                if nb > 1:
                    while True:
                        tree += 1
                        nb = (nb + F - 1) // F
                        if nb <= 1:
                            break
            else:
                nb = tiles
                while True:
                    tree += 1
                    nb = (nb + F - 1) // F
                    if nb <= 1:
                        break
        panels.append((tiles, last_units, tree))
    return pair, rpl, panels


def _next_bw(kp: int, r0: int) -> int:
    left = kp - (r0 + PB)
    return 0 if left <= 0 else min(left, PB)


def _block_forms(kernel: str, kp: int, n2: int, k: int, win: int, pair_flag: int, skip_rhs: bool, sub0: int, subn: int, ny_cols: int):
    """v4_setup + the form choice of the block kernels for ONE problem (kp, n2) in a level-0 launch of panel k: None when the
    problem leaves the launch at once, else the form of every column block of the grid ('full' | 'le16' | 'masked' | 'empty')."""
    r0 = k * PB
    if r0 >= kp:
        return None
    bw = min(kp - r0, PB)
    bwn = _next_bw(kp, r0) if (win or pair_flag) else 0
    if kernel == "pair" and bwn == 0:
        return None
    if kernel == "plain" and pair_flag == 2 and bwn > 0:
        return None
    ncols = n2 + 1 - (r0 + bw) - (1 if skip_rhs else 0)
    if win == 2:
        ncols -= bwn
    ncols -= sub0
    if subn > 0 and ncols > subn:
        ncols = subn
    forms = []
    for yb in range(ny_cols):
        rem = ncols - yb * CW
        if rem <= 0:
            forms.append("empty")
        elif rem >= 32 and bw == PB and (kernel != "pair" or bwn == PB):
            forms.append("full")
        elif rem <= 16:
            forms.append("le16")
        else:
            forms.append("masked")
    return dict(bw=bw, bw2=bwn, ncols=ncols, forms=forms)


def sweep_trace(batch: int, m: int, n: int, t_list, env: dict, tile_rows: int = 512) -> list:
    """The level-0 window-update launches of run_caqr for a batch whose problem i has t_list[i] active constraints of full rank
    (an int: the same for all), on a handle created under `env` with `tile_rows`.  One dict per launch:
      kind 'pair' | 'single' | 'companion' (the pair == 2 launch of a mixed batch) | 'passenger' (no launch: d rides),
      panel, bw, bwb, ntrail, nfar, window (sub0, subn, ncols, has_rhs), stream 'A' | 'B', skip_rhs, ny (grid y extent), ncb
      (column blocks of the grid), tiles, nvu_last (valid 32-row units of the last tile), xmap (tiles, 0: off), xpad (padding
      workgroups of the last octet), tree (tree levels of the step), mixed, lookahead,
      problems: per distinct (kp, n2) of the batch what _block_forms says, and whether its right-hand-side block runs."""
    ts = [int(t_list)] * batch if isinstance(t_list, int) else [int(t) for t in t_list]
    assert len(ts) == batch
    kA = min(n, max(ts))
    pair, rpl, panels = _levels(m, n, kA, batch, tile_rows, env)
    n2s = [n - min(n, t) for t in ts]
    n2_launch = max(n2s)
    mixed = n2_launch != n - kA
    kp_launch = min(m, n2_launch)
    npan = (kp_launch + PB - 1) // PB
    mpad = _rup(max(m, 1), 32)
    la_env = env.get("ENLSIP_GN_LOOKAHEAD", "")
    la_forced = la_env == "1"
    far_wgs0 = batch * ((mpad + 64 * rpl - 1) // (64 * rpl)) * ((n2_launch + 31) // 32)
    la = pair and la_env != "0" and not mixed and ((batch <= LA_MAX_BATCH and far_wgs0 >= LA_MIN_WGS) or la_forced)
    lap = (not pair) and la_env != "0" and not mixed and npan >= 3 and la_forced
    shapes = sorted({(min(m, n2), n2) for n2 in n2s}, reverse=True)
    out = []

    def launch(kind, kernel, k, bw, bwb, ntrail, nfar, ntot, sub0, subn, stream, ngrid_cols, pair_flag, win):
        ncols = min(subn, ntot - sub0) if subn > 0 else ntot - sub0
        has_rhs = sub0 + ncols == ntot
        skip_rhs = has_rhs and (ncols - 1) % 32 == 0
        if ngrid_cols is None:
            ngrid_cols = ncols
        if skip_rhs:
            ngrid_cols -= 1
        ncb = (ngrid_cols + CW - 1) // CW
        tiles, last_units, tree = panels[k]
        xmap = tiles if (kernel == "pair" and batch <= XMAP_MAX_BATCH and tiles >= XMAP_MIN_TILES and not mixed) else 0
        probs = []
        for kp, n2 in shapes:
            f = _block_forms(kernel, kp, n2, k, win, pair_flag, skip_rhs, sub0, subn, ncb)
            if f is not None:
                f.update(kp=kp, n2=n2, rhs_block=skip_rhs)
                probs.append(f)
        out.append(dict(kind=kind, panel=k, bw=bw, bwb=bwb, ntrail=ntrail, nfar=nfar, window=(sub0, subn, ncols, has_rhs),
                        stream=stream, skip_rhs=skip_rhs, ny=ncb + (1 if skip_rhs else 0), ncb=ncb, tiles=tiles, nvu_last=last_units,
                        xmap=xmap, xpad=(8 * ((tiles + 7) // 8) - tiles) if xmap else 0, tree=tree, mixed=mixed,
                        lookahead=la or lap, batch=batch, rpl=rpl, problems=probs))

    def two_streams(ntot, near, update):
        if ntot <= near:
            update(0, 0, "A")
        else:
            update(0, near, "A")
            update(near, 0, "B")

    k = 0
    while k < npan:
        bwk = min(PB, kp_launch - k * PB)
        ntrail = n2_launch + 1 - (k * PB + bwk)
        if pair and not (k & 1) and k + 1 < npan:
            bwb = min(PB, kp_launch - (k + 1) * PB)
            nfar = ntrail - bwb

            def far_update(sub0, subn, stream, k=k, bwk=bwk, bwb=bwb, ntrail=ntrail, nfar=nfar):
                grid_cols = ntrail if mixed else None
                launch("pair", "pair", k, bwk, bwb, ntrail, nfar, nfar, sub0, subn, stream, grid_cols, 1, 2)
                if mixed:
                    launch("companion", "plain", k, bwk, bwb, ntrail, nfar, nfar, sub0, subn, stream, ntrail, 2, 2)

            if la:
                two_streams(nfar, NEAR_PAIR * PB, far_update)
            else:
                far_update(0, 0, "A")
            k += 2
            continue
        passenger = ntrail == 1 and bwk < PB and kp_launch == n2_launch
        if passenger or ntrail <= 0:
            tiles, last_units, tree = panels[k]
            out.append(dict(kind="passenger" if passenger else "none", panel=k, bw=bwk, bwb=0, ntrail=ntrail, nfar=0, tiles=tiles,
                            nvu_last=last_units, tree=tree, mixed=mixed, lookahead=la or lap, batch=batch, rpl=rpl, problems=[],
                            xmap=0, xpad=0, skip_rhs=False, ny=0, ncb=0, window=(0, 0, 0, False), stream="A"))
            k += 1
            continue

        def level_update(sub0, subn, stream, k=k, bwk=bwk, ntrail=ntrail):
            launch("single", "plain", k, bwk, 0, ntrail, 0, ntrail, sub0, subn, stream, None, 0, 0)

        if lap:
            two_streams(ntrail, NEAR_PLAIN * PB, level_update)
        else:
            level_update(0, 0, "A")
        k += 1
    return out


def expected_sweep_route(trace: list, env: dict) -> tuple:
    """(bits the solve must report, sweep bits it must NOT report) of a trace."""
    sweep = {"sweep_plain", "sweep_pairs", "sweep_passenger", "sweep_tree", "sweep_lookahead", "sweep_xmap"}
    want = set()
    for L in trace:
        if L["kind"] == "pair":
            want.add("sweep_pairs")
        elif L["kind"] in ("single", "none"):
            want.add("sweep_plain")
        elif L["kind"] == "passenger":
            want.add("sweep_passenger")
        if L["tree"] > 0:
            want.add("sweep_tree")
        if L["xmap"]:
            want.add("sweep_xmap")
        if L["lookahead"]:
            want.add("sweep_lookahead")
    return want, sweep - want


# ---- edge names -------------------------------------------------------------------------------------------------------------------
def edges(c: dict, trace: list) -> set:
    """Names of the edge values the trace of case c contains, by family (a case only speaks for its own family, and for the
    family-free kernel branches `form.*` / `rhs.*`)."""
    fam = c["family"]
    out = set()
    pairs = [L for L in trace if L["kind"] == "pair"]
    for L in trace:
        if L["kind"] in ("passenger", "none"):
            continue
        kern = "pair" if L["kind"] == "pair" else "plain"
        for P in L["problems"]:
            for f in P["forms"]:
                if f != "empty":
                    out.add(f"form.{kern}.{f}")
            if L["skip_rhs"]:
                out.add(f"rhs.own_block.{kern}")
                if L["ncb"] == 0:
                    out.add(f"rhs.alone.{kern}")
                if kern == "pair" and P["bw2"] < PB:
                    out.add("rhs.own_block.pair.narrow_second")
            elif L["window"][3] and P["forms"]:
                last = P["ncols"] - CW * ((P["ncols"] - 1) // CW)          # the right-hand side's position in its block
                if last in (2, 17, 32):
                    out.add(f"rhs.rides.col{last}")
            if kern == "pair" and P["bw2"] < PB and any(f in ("le16", "masked") for f in P["forms"]):
                out.add("form.pair.narrow_second")
    if fam == "A" and pairs:
        npan = max(L["panel"] for L in trace) + 1 + (1 if trace[-1]["kind"] == "pair" else 0)
        last = pairs[-1]
        out.add(f"A.q={c['q']}")
        if npan % 2 == 1:
            out.add(f"A.odd.nfar={last['nfar']}")
            out.add(f"A.odd.last={trace[-1]['kind']}")
        else:
            assert last["nfar"] == 1
            out.add(f"A.even.bw2={last['bwb']}")
            out.add(f"A.even.prev_nfar={pairs[-2]['nfar']}")
            if pairs[-2]["skip_rhs"]:
                out.add("A.even.prev_skip_rhs")
    if fam in ("A", "B") and pairs:
        L = pairs[0]
        rows = "wide" if c["m"] < c["n"] - c["t"] else f"{c['m'] // (64 * L['rpl'])}x+{c['m'] % (64 * L['rpl'])}"
        out.add(f"B.tile{64 * L['rpl']}.m={rows}")
        out.add(f"B.nvu_last={L['nvu_last']}")
        if L["tiles"] == 1:
            out.add("B.one_tile_pair")
        if L["tiles"] > 1 and L["nvu_last"] == 1:
            out.add("B.last_tile_without_second_panel_rows")
        if c["m"] < c["n"] - c["t"] and trace[-1]["kind"] == "single" and trace[-1]["bw"] < PB:
            out.add("B.wide.narrow_last_panel_not_passenger")
    if fam == "C" and pairs:
        L = pairs[0]
        out.add(f"C.tile{64 * L['rpl']}.tiles={L['tiles']}")
        out.add(f"C.batch={L['batch']}.xmap={'on' if L['xmap'] else 'off'}")
        if L["xmap"]:
            out.add(f"C.xpad={L['xpad']}")
        if L["xmap"] and L["tiles"] % 8 == 1 and c["m"] - 64 * L["rpl"] * (L["tiles"] - 1) >= 64:
            out.add(f"C.tiles={L['tiles']}.last_tile_two_full_units")
        if L["xmap"] and c["m"] % (64 * L["rpl"]) == 1:
            out.add(f"C.tile{64 * L['rpl']}.tiles={L['tiles']}.last_tile_one_row")
        for L in pairs:
            out.add(f"C.ny={L['ny']}.rhs_last={int(L['skip_rhs'])}")
    if fam == "D":
        for L in trace:
            if not L["lookahead"]:
                continue
            if L["kind"] == "pair" and L["window"][0] == 0:
                out.add(f"D.pair.nfar={L['nfar']}")
                if L["window"][1] == 0:
                    out.add("D.pair.one_part")
            if L["kind"] == "pair" and L["window"][0] > 0 and L["ncb"] == 0:
                out.add("D.pair.rest_is_rhs_alone")
            if L["kind"] == "single" and L["window"][0] == 0:
                out.add(f"D.plain.ntrail={L['ntrail']}")
            if L["kind"] == "pair" and L["xmap"] and L["window"][0] > 0:
                out.add("D.pair.subwindow_meets_xmap")
    if fam == "E":
        for L in trace:
            if not L["mixed"] or L["kind"] not in ("pair", "companion"):
                continue
            tag = f"E.tiles={L['tiles']}.skip_rhs={int(L['skip_rhs'])}"
            r0 = L["panel"] * PB
            for P in L["problems"]:
                if L["kind"] == "companion" and P["n2"] == r0 + PB:
                    out.add(f"{tag}.ends_at_first_panel")
                if L["kind"] == "pair" and r0 + PB < P["n2"] < r0 + 2 * PB:
                    out.add(f"{tag}.ends_inside_second_panel")
                if L["kind"] == "pair" and P["n2"] == max(q["n2"] for q in L["problems"]) and P["bw2"] == PB:
                    out.add(f"{tag}.launch_width")
    return out


A_ODD = (1, 15, 16, 17, 31, 32)           # kp = n2 = 64 q + r: odd panel count, last pair's nfar = r + 1
A_EVEN = (33, 47, 48, 63, 64)             # even panel count: second panel of the last pair r - 32 wide, the pair before: nfar = r + 1
B_OFFSETS = (0, 1, 31, 32, 33, 511)
C_ROWS = (7680, 8192, 8193, 11776, 12288, 12289)
D_PAIR_NFAR = (64, 65, 66, 96, 97)
D_PLAIN_NTRAIL = (32, 33, 34, 65)


def required_edges() -> set:
    """Every edge value families A to E name (the issue's list), in the vocabulary of edges()."""
    req = {f"form.{k}.{f}" for k in ("pair", "plain") for f in ("full", "le16", "masked")}
    req |= {"rhs.own_block.pair", "rhs.own_block.plain", "rhs.alone.pair", "rhs.own_block.pair.narrow_second", "rhs.rides.col2",
            "rhs.rides.col17", "rhs.rides.col32", "form.pair.narrow_second"}
    req |= {f"A.q={q}" for q in (1, 2)}
    req |= {f"A.odd.nfar={r + 1}" for r in A_ODD} | {"A.odd.last=passenger", "A.odd.last=single"}
    req |= {f"A.even.bw2={r - 32}" for r in A_EVEN} | {f"A.even.prev_nfar={r + 1}" for r in A_EVEN} | {"A.even.prev_skip_rhs"}
    req |= {f"B.tile512.m={g}x+{o}" for g in (1, 2) for o in B_OFFSETS}
    req |= {f"B.tile256.m={(512 + o) // 256}x+{(512 + o) % 256}" for o in B_OFFSETS}
    req |= {"B.tile256.m=wide", "B.nvu_last=1", "B.nvu_last=2", "B.nvu_last=16", "B.nvu_last=8", "B.one_tile_pair",
            "B.last_tile_without_second_panel_rows", "B.wide.narrow_last_panel_not_passenger"}
    req |= {f"C.tile512.tiles={(m + 511) // 512}" for m in C_ROWS} | {"C.tile256.tiles=16", "C.tile256.tiles=17"}
    req |= {"C.batch=1.xmap=on", "C.batch=2.xmap=on", "C.batch=8.xmap=on", "C.batch=9.xmap=off", "C.batch=1.xmap=off"}
    req |= {f"C.xpad={p}" for p in (0, 7, 1)}
    # one tile into an octet with ONE real row in it (8193, 12289 rows) that tile's reflectors are the identity and dropping the tile
    # changes nothing: the same tile counts again with 64 real rows in the last tile
    req |= {"C.tiles=17.last_tile_two_full_units", "C.tiles=25.last_tile_two_full_units"}
    req |= {"C.tile512.tiles=17.last_tile_one_row", "C.tile512.tiles=25.last_tile_one_row", "C.tile256.tiles=17.last_tile_one_row"}
    req |= {f"C.ny={ny}.rhs_last={r}" for ny in (1, 2, 3) for r in (0, 1)}
    req |= {f"D.pair.nfar={v}" for v in D_PAIR_NFAR} | {f"D.plain.ntrail={v}" for v in D_PLAIN_NTRAIL}
    req |= {"D.pair.one_part", "D.pair.rest_is_rhs_alone", "D.pair.subwindow_meets_xmap"}
    req |= {f"E.tiles={tl}.skip_rhs={s}.{what}" for tl in (1, 3) for s in (0, 1)
            for what in ("ends_at_first_panel", "ends_inside_second_panel", "launch_width")}
    return req


# ---- the table --------------------------------------------------------------------------------------------------------------------
PAIRS = {"ENLSIP_GN_PAIR": "1", "ENLSIP_GN_LOOKAHEAD": "0"}


def _mk(family, tag, batch, m, n, t, env, tile_rows=0, t_list=None, q=0):
    tl = f"-t{'.'.join(map(str, t_list))}" if t_list else f"-t{t}"
    c = dict(id=f"{family}-{tag}-b{batch}-{m}x{n}{tl}" + (f"-tile{tile_rows}" if tile_rows else ""), family=family, batch=batch,
             m=m, n=n, t=max(t_list) if t_list else t, t_list=t_list, env=dict(env), tile_rows=tile_rows, q=q)
    assert m * n <= SIZE_CAP and batch <= BATCH_CAP, c["id"]
    return c


def trace_of(c: dict) -> list:
    return sweep_trace(c["batch"], c["m"], c["n"], c["t_list"] if c["t_list"] else c["t"], c["env"], c["tile_rows"] or 512)


def cases() -> list:
    """The table (dicts: id, family, batch, m, n, t, t_list, env, tile_rows).  Families A and B share their cases: the far-window
    widths of A take their row counts from B's list, so that neither family pays a case of its own for what the other leaves free."""
    out = []
    t = 3
    rows = [512 * g + o for g in (1, 2) for o in B_OFFSETS]
    # A (+ B's 512-row tiles): n2 = 64 q + r, q alternating, on the row counts 512 g + offset
    for i, r in enumerate(A_ODD + A_EVEN):
        q = 1 + i % 2
        out.append(_mk("A", f"r{r}", 1, rows[i], 64 * q + r + t, t, PAIRS, q=q))
    # B: the row count A left over, the same offsets on 256-row tiles, a one-tile pair of 256-row-tile size, a wide problem
    for m in rows[len(A_ODD + A_EVEN):]:
        out.append(_mk("B", "rows", 1, m, 68 + t, t, PAIRS))
    for o in B_OFFSETS:
        out.append(_mk("B", "rows", 1, 512 + o, 68 + t, t, PAIRS, tile_rows=256))
    out.append(_mk("B", "wide", 1, 70, 200 + t, t, PAIRS))
    # C: 15 .. 25 tiles, batches 1 | 2 | 8 | 9, far grids of 1, 2, 3 block indices with and without the right-hand-side block last
    n2_by_grid = {(2, 1): 96, (1, 0): 80, (2, 0): 100, (3, 1): 128, (3, 0): 140}      # n2 -> (ny, rhs block last) of the first pair
    plan = [(7680, 1, (1, 0)), (8192, 8, (2, 1)), (8193, 2, (2, 0)), (11776, 1, (3, 1)), (12288, 1, (3, 0)), (12289, 1, (1, 0))]
    for m, b, grid in plan:
        out.append(_mk("C", "octet", b, m, n2_by_grid[grid] + t, t, PAIRS))
    out.append(_mk("C", "octet", 9, 8192, 96 + t, t, PAIRS))
    out.append(_mk("C", "octet", 1, 8192 + 64, 80 + t, t, PAIRS))
    out.append(_mk("C", "octet", 1, 12288 + 64, 80 + t, t, PAIRS))
    out.append(_mk("C", "octet", 1, 4096, 96 + t, t, PAIRS, tile_rows=256))
    out.append(_mk("C", "octet", 2, 4097, 80 + t, t, PAIRS, tile_rows=256))
    # D: look-ahead forced; first pair's nfar = n2 + 1 - 64, plain sweep's ntrail = n2 + 1 - 32 (k + 1)
    la_pairs = {"ENLSIP_GN_PAIR": "1", "ENLSIP_GN_LOOKAHEAD": "1"}
    la_plain = {"ENLSIP_GN_PAIR": "0", "ENLSIP_GN_LOOKAHEAD": "1"}
    for nfar in D_PAIR_NFAR:
        out.append(_mk("D", "pairs", 1, 600, nfar + 63 + t, t, la_pairs))
    for n2 in (95, 96, 97):
        out.append(_mk("D", "plain", 1, 600, n2 + t, t, la_plain))
    out.append(_mk("D", "octet", 1, 8193, 130 + t, t, la_pairs))
    # E: mixed widths under forced pairs, one tile and three
    for m in (400, 1100):
        out.append(_mk("E", "mixed", 3, m, 100, 0, PAIRS, t_list=[4, 40, 68]))
        out.append(_mk("E", "mixed", 4, m, 101, 0, PAIRS, t_list=[4, 5, 41, 69]))
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), ids
    return out


def covered(cs=None) -> set:
    out = set()
    for c in (cases() if cs is None else cs):
        out |= edges(c, trace_of(c))
    return out


def problem(c: dict, k: int):
    """(J, rx, A, cx) of problem k of case c: synth.make_problem, a seed per case and problem."""
    from oracle import synth
    tk = c["t_list"][k] if c["t_list"] else c["t"]
    return synth.make_problem(problem_seed(c, k), c["m"], c["n"], tk)


def problem_seed(c: dict, k: int) -> int:
    import factor_identities as fi
    return 91000 + 131 * (fi.hash_id(f"{c['m']}x{c['n']}-{c['t']}-{c['tile_rows']}") % 1000) + k
