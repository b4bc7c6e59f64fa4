"""CPU checks of tests/conv_sk_forms.py, the host mirror of `launch_conv_sk`, and of the conv_sk / XCD cases of
tests/test_hip_conv_kernels.py that lean on it:
  * the union of the forms the `kern = 7` cases reach covers every instantiation and every K-pass shape the launcher can pick;
  * the cases from before the forms were listed still report the one form they always ran (NJ = 1, one pass per source, cpu_ <= 4);
  * `sk_tile` against a brute-force search of the kernel's tile rule over every map of at most 4096 pixels;
  * a float64 emulation of the kernel's decomposition (conv_sk_forms.emulate) holds the per-element bound on every new case's own
    operands, and each of eight deliberate defects of that decomposition exceeds it on a case that reaches the form the defect needs.

The operands are the GPU test's: `_make_case` itself runs here, with `Tensor.cuda()` made the identity and the producer launch of the
`gn = "st"` cases replaced by its float64 reference rounded to the storage type (same generator draws, same shapes)."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import conv_sk_forms as skf
import test_hip_conv_kernels as tc
from test_hip_conv_kernels import CASES, FORMS, N_CASES_ONE_FORM, XCD_TILES, _bound, conv_reference, gn_coef_reference, q

SK = [i for i, c in enumerate(CASES) if c["kern"] == 7]
NEW = [i for i in SK if i >= N_CASES_ONE_FORM]
OLD = [i for i in SK if i < N_CASES_ONE_FORM]


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_read_from_the_source_and_a_lost_pattern_is_loud():
    k = skf.constants()
    assert k["SK_MT"] >= 32 and k["SK_HPMAX"] >= k["SK_MT"] and k["WIDE_WGS"] > 0 and k["MAX_PX"] > 0 and k["MAX_PX_F32"] >= k["MAX_PX"]
    assert set(k["CP"]) == {(dt, nj) for dt in (0, 1, 2) for nj in (1, 2)} and set(k["CP_HEAD"]) == {(1, 1), (2, 1)}
    assert all(cp % 32 == 0 for cp in list(k["CP"].values()) + list(k["CP_HEAD"].values()))
    with pytest.raises(AssertionError, match="the launcher changed"):
        skf._one("use_conv_sk.hip", r"constexpr int SK_NO_SUCH_LINE = (\d+);", "a line that is not there")


def test_sk_tile_is_the_kernels_rule_by_brute_force():
    """Every H, W with H W <= 4096, 3x3 and 1x1: TH TW <= SK_MT, halo <= SK_HPMAX, and no admissible shape needs fewer tiles."""
    k = skf.constants()
    MT, HP = k["SK_MT"], k["SK_HPMAX"]
    hh, ww = np.meshgrid(np.arange(1, MT + 1), np.arange(1, MT + 1), indexing="ij")
    ok = hh * ww <= MT
    hh, ww = hh[ok], ww[ok]
    n = 0
    for pad in (0, 1):
        adm = (hh + 2 * pad) * (ww + 2 * pad) <= HP
        ah, aw = hh[adm], ww[adm]
        for H in range(1, 4097):
            Ws = np.arange(1, 4096 // H + 1)
            # shapes clipped to the map: a tile beyond the map covers no more and has no smaller halo
            fits = (ah[None, :] <= H) & (aw[None, :] <= Ws[:, None])
            tiles = -(-H // ah[None, :]) * -(-Ws[:, None] // aw[None, :])
            fewest = np.where(fits, tiles, 1 << 30).min(1)
            for W, best in zip(Ws.tolist(), fewest.tolist()):
                th, tw = skf.sk_tile(H, W, pad)
                assert 1 <= th <= H and 1 <= tw <= W and th * tw <= MT and (th + 2 * pad) * (tw + 2 * pad) <= HP, (H, W, pad, th, tw)
                assert -(-H // th) * -(-W // tw) == best, (H, W, pad, th, tw, best)
                n += 1
    print(f"[sk_tile] {n} maps: tile within {MT} px, halo within {HP} px, fewest tiles")


def test_tall_maps_of_one_or_two_columns_get_halo_capped_tiles():
    """What the brute-force search found: on these maps the tallest tile of every width exceeds the halo and the first round of sk_tile finds
    nothing (it used to leave one-pixel tiles: 128 workgroups per channel tile on 64 x 2); the second round caps the height by the halo."""
    assert skf.sk_tile(64, 2, 1) == (22, 2) and skf.sk_tile(41, 1, 1) == (21, 1) and skf.sk_tile(64, 1, 1) == (32, 1)
    assert skf.sk_tile(64, 2, 0) == (64, 1) and skf.sk_tile(40, 1, 1) == (40, 1) and skf.sk_tile(32, 2, 1) == (32, 1)      # first round, as before
    assert skf.sk_tile(16, 20, 1) == (16, 4) and skf.sk_tile(8, 10, 1) == (8, 5) and skf.sk_tile(64, 64, 1) == (8, 8)


def test_cases_from_before_keep_their_one_form():
    """The finding this file pins: every conv_sk case that existed before ran NJ = 1 with one K pass per source and cpu_ <= 4, on W >= 9."""
    for i in OLD:
        NJ, CP, tiles, wgs, passes = skf.sk_form(CASES[i])
        assert NJ == 1 and all(len(p) == 1 and 1 <= p[0] <= 4 for p in passes) and CASES[i]["W"] >= 9, (i, NJ, CP, passes)
        assert wgs <= skf.constants()["WIDE_WGS"]
    assert len(OLD) == 22 and not any(i in FORMS for i in OLD)


def test_the_cases_cover_every_form_the_launcher_picks():
    k = skf.constants()
    reached = {}                                   # (dt, odt != dt, NJ) -> set of cpu_
    facts = set()
    for i in SK:
        c = CASES[i]
        assert skf.sk_eligible(c), i
        NJ, CP, tiles, wgs, passes = skf.sk_form(c)
        head = c.get("odt", c["dt"]) != c["dt"]
        reached.setdefault((c["dt"], head, NJ), set()).update(p for src in passes for p in src)
        plist = skf.sk_passes(c, CP)
        multi = any(len(src) > 1 for src in passes)
        if any(c_loc > 0 for _, _, c_loc, _ in plist):
            facts.add("c_loc > 0")
            if c.get("ntaps", 9) == 9:
                facts.add("3x3 with c_loc > 0")
        if any(len(src) > 1 and src[-1] < CP // 32 for src in passes):
            facts.add("partial last pass")
        if multi and any(cg0 > 0 for _, cg0, _, _ in plist):
            facts.add("second source with cg0 > 0 in a multi-pass case")
        if NJ == 2:
            facts.add(f"NJ 2 {skf.weight_branch(c)[0]}")
        if c["W"] <= 2:
            facts.add(f"W = {c['W']}")
        if not head and c["Cout"] % 64 == 0:
            facts.add("at the seam, narrow" if wgs == k["WIDE_WGS"] else "past the seam, wide" if k["WIDE_WGS"] < wgs <= 2 * k["WIDE_WGS"] else "")
        if not head and c["Cout"] % 64 and wgs > k["WIDE_WGS"]:
            facts.add("Cout % 64 != 0 above the threshold")
    want = {}
    for (dt, nj), cp in k["CP"].items():
        want[(dt, False, nj)] = set(range(1, cp // 32 + 1))
    for (dt, nj), cp in k["CP_HEAD"].items():
        want[(dt, True, nj)] = {2, 4, 8}           # the heads: a whole pass, a partial pass (every cpu_ runs under the same-type NJ 1 form)
    for key in sorted(want):
        print(f"[forms] {tc.DT_NAME[key[0]]}{' -> fp32 head' if key[1] else ''} NJ {key[2]}: cpu_ reached {sorted(reached.get(key, ()))}")
    missing = {key: sorted(v - reached.get(key, set())) for key, v in want.items() if v - reached.get(key, set())}
    assert not missing, f"forms no case reaches: {missing}"
    need = {"c_loc > 0", "3x3 with c_loc > 0", "partial last pass", "second source with cg0 > 0 in a multi-pass case", "NJ 2 slab", "NJ 2 row",
            "W = 1", "W = 2", "at the seam, narrow", "past the seam, wide", "Cout % 64 != 0 above the threshold"}
    print(f"[forms] {sorted(facts - {''})}")
    assert need <= facts, need - facts
    # every new case states its form, and every XCD case has a grid the re-ordering applies to
    assert sorted(FORMS) == NEW
    for c in CASES:
        tc._assert_form(c)
    assert sorted(skf.xcd_tile(b, 16) for b in range(16)) == list(range(16)) and [skf.xcd_tile(b, 16) for b in range(3)] == [0, 2, 4]
    assert [skf.xcd_tile(b, 8) for b in range(8)] == list(range(8)) and [skf.xcd_tile(b, 6) for b in range(6)] == list(range(6))
    assert sorted(set(XCD_TILES.values())) == [8, 16]


def test_unit_walk_visits_every_unit_once():
    """The division-free stepping reaches each (tap, chunk) exactly once for every cpu_ and both tap counts."""
    for wtaps in (1, 9):
        for cpu_ in range(1, 9):
            m = skf.unit_walk(wtaps, cpu_)
            assert all(v == 1 for row in m for v in row), (wtaps, cpu_, m)


# ---- the cases' own operands on the CPU -------------------------------------------------------------------------------------------
def _cpu_producer(g, B, H, W, Cc, dt):
    """`_producer` without a device: the same draws, the 1x1 convolution in float64, rounded to the storage type."""
    prev = tc._border_heavy(g, B, H, W, 32, dt)
    w = torch.randn(Cc, 32, generator=g) * 0.3
    bias = torch.randn(Cc, generator=g) * 0.5
    y, _ = conv_reference(prev, None, 0, w, dt, bias=bias)
    out = q(y, dt)
    return out, out.to(tc.TD[dt]), None


@functools.lru_cache(None)
def _host_case(i):
    c = CASES[i]
    with mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self), mock.patch.object(tc, "_producer", _cpu_producer):
        f, ref, S, creal = tc._make_case(c, seed=len(tc._case_id(c)) * 7919 + i)
    B, Cout = f["B"], f["Cout"]
    src = torch.cat([f["d_src0"].double()] + ([f["d_src1"].double()] if f["C1"] else []), -1)
    coef = None
    if f["gn"] == "coef":
        coef = f["d_coef"].double()
    elif f["gn"] == "st":
        coef = gn_coef_reference(src, f["d_gamma"], f["d_beta"], f["groups"])
    temb = None
    if f["d_temb"] is not None:
        temb = f["d_temb"][:1].expand(B, Cout) if f["temb_bstride"] < 0 else f["d_temb"][:, :Cout]
    ops = dict(q=q, src=src, coef=coef, act=f["act"], w=torch.from_numpy(f["h_w"]), bias=torch.from_numpy(f["h_bias"]), temb=temb,
               res=None if f["d_res"] is None else f["d_res"].double(), scale=f["scale"])
    if f["XC0"]:
        ops["xs"] = torch.cat([f["d_x0"].double()] + ([f["d_x1"].double()] if f["XC1"] else []), -1)
        ops["w2"] = torch.from_numpy(f["h_w2"])
    if f["d_pyr"] is not None:
        ops["pyr"], ops["w4"], ops["b4"] = f["d_pyr"].double(), torch.from_numpy(f["h_w4"]), torch.from_numpy(f["h_b4"])
    return c, f, ref, S, creal, ops


def _ratio(i, got):
    """Worst |got - ref| / bound of case i, as the GPU test forms it."""
    c, f, ref, S, creal, _ = _host_case(i)
    K = (f["C0"] + f["C1"]) * f["ntaps"] + f["XC0"] + f["XC1"]
    bound = _bound(ref[..., :creal], S[..., :creal], c["dt"], f["odt"], f["scale"], K)
    return float(((got[..., :creal] - ref[..., :creal]).abs() / bound).max())


@pytest.mark.parametrize("i", NEW, ids=[tc._case_id(CASES[i]).split("-gn")[0].split("-temb")[0] for i in NEW])
def test_emulation_holds_the_bound_on_every_new_case(i):
    """The unmutated decomposition - pass loop, offsets, unit walk, channel tiles, store rounding - is within the per-element bound."""
    c, f, ref, S, creal, ops = _host_case(i)
    got, _ = skf.emulate(c, ops)
    r = _ratio(i, got)
    print(f"[emulation] case {i} {tc._case_id(c)}: form {skf.sk_form(c)} err/bound {r:.3f}")
    assert r < 1.0
    assert creal == f["Cout"] or float(got[..., creal:].abs().max()) == 0.0


def _first(**want):
    """Index of the first new case with the given dt whose form has the given NJ."""
    for i in NEW:
        c = CASES[i]
        if all((skf.sk_form(c)[0] if k == "NJ" else c.get(k, 0)) == v for k, v in want.items()):
            return i
    raise AssertionError(want)


# the defects and the (small) cases each is tried on: 16-bit and fp32, NJ 1 and NJ 2, 3x3 and 1x1
DEFECTS = {
    "drop_pass2": "the second pass dropped",
    "halo_no_cloc": "the second pass reading the first pass's channels (c_loc ignored in the halo load)",
    "weights_no_cloc": "the second pass under the first pass's weights",
    "table_no_cglob": "the GroupNorm table read without c_glob",
    "j1_as_j0": "channel tile j = 1 under j = 0's weights",
    "skip_unit": "one (tap, chunk) unit skipped for a non-power-of-two cpu_",
    "repeat_tap": "the last tap of a wave's walk repeated",
}


def _defect_cases():
    pick = [_first(dt=1, H=16, W=20, C0=224),              # A   bf16 NJ 1 [7] [5] [6]
            _first(dt=2, H=8, W=10, C0=384),               # B2  fp16 NJ 1 [8, 4]
            _first(dt=1, H=16, W=2, C0=1024),              # B3  bf16 NJ 1 four passes, W = 2
            _first(dt=1, H=8, W=10, C0=160, NJ=2),         # C2  bf16 NJ 2 [4, 1] [3] [2]
            _first(dt=2, H=8, W=10, ntaps=1, NJ=2),        # C3  fp16 NJ 2 1x1, row-major weights
            _first(dt=1, Cout=4),                          # H   bf16 head [8, 4]
            _first(dt=0, H=16, W=20, C0=256),              # D1  fp32 NJ 1 [4, 4]
            _first(dt=0, H=7, W=9, C0=160),                # D2  fp32 NJ 1 [4, 1] [3] [4, 1]
            _first(dt=0, H=64, W=16, NJ=2),                # E2  fp32 NJ 2 [2, 1] [2] [2, 1]
            _first(dt=0, H=8, W=10, ntaps=1, NJ=2)]        # fp32 NJ 2 1x1, four passes
    assert len(set(pick)) == len(pick)
    return pick


@pytest.mark.parametrize("mutant", list(DEFECTS))
def test_each_defect_of_the_decomposition_exceeds_the_bound(mutant):
    """A defect counts on the cases whose form it needs (a second pass, c_glob > 0 under a GroupNorm, NJ = 2, a cpu_ that is no power of
    two, a 3x3 walk); on every one of them it must exceed the bound the kernel is held to."""
    ratios = {}
    for i in _defect_cases():
        c, f, ref, S, creal, ops = _host_case(i)
        got, hit = skf.emulate(c, ops, mutant)
        if hit:
            ratios[i] = _ratio(i, got)
    print(f"[defect] {DEFECTS[mutant]}: " + ", ".join(f"case {i} ({tc.DT_NAME[CASES[i]['dt']]} NJ {skf.sk_form(CASES[i])[0]}) {r:.3g}" for i, r in ratios.items()))
    forms = {(CASES[i]["dt"] != 0, skf.sk_form(CASES[i])[0]) for i in ratios}
    assert len(ratios) >= 2 and (mutant != "j1_as_j0" or forms == {(True, 2), (False, 2)})
    assert min(ratios.values()) > 1.0, ratios


@pytest.mark.parametrize("i", [i for i, n in XCD_TILES.items() if n == 8], ids=lambda i: tc._case_id(CASES[i]).split("-gn")[0])
def test_a_transposed_tile_list_exceeds_the_bound_on_the_xcd_cases(i):
    """The 8-tile grids: every workgroup computing the tile of the transposed list (2 x 4 read as 4 x 2) moves six of eight tiles."""
    c, f, ref, S, creal, _ = _host_case(i)
    k = skf.constants()
    th, tw = (k["V2_T"], k["V2_T"]) if c["kern"] == 2 else (k["V4_TH"], k["V4_TW"])
    good = q(ref, f["odt"])
    r0, r1 = _ratio(i, good), _ratio(i, skf.transpose_tiles(good, th, tw))
    print(f"[defect] the tile list of an 8-tile grid transposed: case {i} {tc.KERNEL[c['kern']]} {tc.DT_NAME[c['dt']]} {r1:.3g} (untransposed {r0:.3f})")
    assert r0 < 1.0 < r1
