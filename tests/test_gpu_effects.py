"""The variant-effect stage on the device (csrc/hawk_effects.hip behind hawk_effects_*): against the reference's tables
(tests/golden/g14_effects.json.gz) from search -> collapse -> effects on the table in HBM, and against the host twin bit for bit
on the fixtures' groups and on hand-built seam panels (effects_refs.py, which also states the comparison rule)."""
import functools
import os

import numpy as np
import pytest

from crisprhawk_hip import _lib, graphical_reports as gr, reports, synth
from oracle import oracle as ora
import effects_refs as refs

pytestmark = pytest.mark.gpu
TABLES = ["cfdon", "cfdon_two", "cfdon_none_valid", "azimuth", "azimuth_two", "azimuth_nans"]


@functools.lru_cache(maxsize=None)
def device_report(name):
    """search -> collapse on the device, the table kept in HBM; its exported groups and report columns"""
    from crisprhawk_hip.hapset import DeviceHapSet, HostHaplotype
    from util import load_golden
    fx = load_golden(f"g7_report_{name}.json.gz")
    hs, labels = refs.oracle_inputs(fx)
    ds = DeviceHapSet([HostHaplotype(seq, lb.segments, r, sc) for seq, lb, r, sc in zip(hs.seqs, labels, hs.is_ref, hs.scan)])
    bits, bitsrc, _, _ = ora.pam_encode(fx["pam"])
    mm, pt = synth.cfd_tables()
    tab = ds.search(bits, bitsrc, len(fx["pam"]), fx["guidelen"], fx["right"], mm, pt, download=False, collapse=True)
    groups = tab.export_groups()
    lab = reports.HapLabels.from_objects(labels)
    is_ref = np.asarray(ds.is_ref, dtype=bool)
    columns = reports.group_columns(groups, lab, refs.fixture_pam(fx), fx["contig"], fx["target"], with_cfdon=True, is_ref_hap=is_ref)
    assert reports.to_tsv(reports.report_from_groups(groups, lab, refs.fixture_pam(fx), fx["contig"], fx["target"], with_cfdon=True,
                                                     is_ref_hap=is_ref)) == fx["report_tsv"]
    return fx, ds, tab, groups, lab, is_ref, columns


def _args(name, key):
    fx, ds, tab, groups, lab, is_ref, columns = device_report(name)
    rec = refs.g14()["fixtures"][name]
    score = "score_cfdon" if key.startswith("cfdon") else "score_azimuth"
    cg = rec["candidates"][key.split("_", 1)[1]] if "_" in key else []
    scores = {"score_azimuth": refs.group_scores(rec["score_azimuth"], columns[1])} if score == "score_azimuth" else None
    return fx, tab, groups, lab, is_ref, columns, rec, score, cg, scores


@pytest.mark.parametrize("key", TABLES)
def test_device_delta_tables_match_the_reference(key):
    split = 0
    for name in refs.FIXTURES:
        fx, tab, groups, lab, is_ref, columns, rec, score, cg, scores = _args(name, key)
        df = gr.compute_delta_table(tab, lab, cg, score, engine="device", columns=columns, scores=scores, is_ref_hap=is_ref)
        s, _ = refs.compare_table(df, rec["tables"][key], len(cg), fx["report_tsv"])
        split += s
    if key in ("cfdon", "azimuth"):
        assert split <= 1


@pytest.mark.parametrize("name", refs.FIXTURES)
def test_device_type_counts_match_the_reference(name):
    fx, ds, tab, groups, lab, is_ref, columns = device_report(name)
    assert gr.guide_type_counts(tab, lab, columns[1], engine="device", is_ref_hap=is_ref) == refs.g14()["fixtures"][name]["type_counts"]


@pytest.mark.parametrize("name", refs.FIXTURES)
def test_table_route_columns_route_and_host_twin_agree_bit_for_bit(name):
    """hawk_effects_create on the table in HBM, hawk_effects_create_columns on its exported groups, hawk_host_effects on the same"""
    fx, ds, tab, groups, lab, is_ref, columns = device_report(name)
    rec = refs.g14()["fixtures"][name]
    order = columns[1]
    cands = gr.parse_candidate_ids(rec["candidates"]["two"])
    az = refs.group_scores(rec["score_azimuth"], order)
    stages = [gr.GroupEffects(tab, lab.samples, is_ref, order, "device"), gr.GroupEffects(groups, lab.samples, is_ref, order, "device"),
              gr.GroupEffects(groups, lab.samples, is_ref, order, "host")]
    assert stages[1].perm is None  # the export is in collapse order
    try:
        for family, score, cg, K in ((gr.SIGNED, None, (), 25), (gr.SIGNED, None, cands, 25), (gr.ABSOLUTE, az, cands, 25), (gr.ABSOLUTE, az, (), 64)):
            res = [st.rank(family, score, cg, K) for st in stages]
            refs.results_equal(res[0], res[2])
            refs.results_equal(res[1], res[2])
            assert len(res[0].chosen) == min(K, len(cg) + int((res[0].pos_ref != gr.FX_NONE).sum() - len(cg)))
    finally:
        for st in stages:
            st.close()


def _both(panel, order):
    dev = gr.GroupEffects(panel, panel.hap_samples, panel.is_ref_hap, order, "device")
    host = gr.GroupEffects(panel, panel.hap_samples, panel.is_ref_hap, order, "host")
    return dev, host


def _agree(dev, host, family, score, cands, K):
    a, b = dev.rank(family, score, cands, K), host.rank(family, score, cands, K)
    refs.results_equal(a, b)
    return a


@pytest.mark.parametrize("order_kind", ["collapse", "reverse", "random"])
def test_positions_panel_device_equals_host(order_kind):
    """positions of 1, 2, 63, 64, 65 groups, one across every workgroup boundary, 2 workgroups + 1 group; no REF, REF only, REF
    last in collapse order but first in the report; the report in collapse order, reversed, shuffled; K = 1, 25 and 64 (three
    workgroups feed the merge)"""
    p, sizes = refs.positions_panel()
    n = p.n_groups
    assert n == 513
    order = {"collapse": np.arange(n), "reverse": np.arange(n)[::-1].copy(), "random": np.random.default_rng(9).permutation(n)}[order_kind]
    dev, host = _both(p, order)
    rng = np.random.default_rng(10)
    az = np.round(rng.random(n), 4)
    az[rng.random(n) < 0.1] = np.nan
    heads = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    try:
        for K in (1, 25, 64):
            r = _agree(dev, host, gr.SIGNED, None, (), K)
            assert len(r.chosen) == K
            _agree(dev, host, gr.ABSOLUTE, az, (), K)
        with_ref = [int(h) for h in heads if r.pos_ref[h] != gr.FX_NONE]
        cands = [(int(p.start[h]), int(p.strand[h])) for h in (with_ref[-1], with_ref[3], with_ref[40])]
        r = _agree(dev, host, gr.SIGNED, None, cands, 25)
        assert r.chosen[:3].tolist() == [with_ref[-1], with_ref[3], with_ref[40]] and len(set(r.chosen.tolist())) == 25
        r = _agree(dev, host, gr.ABSOLUTE, az, cands + [(1, 0)], 64)   # the last candidate names no position
        assert r.chosen[3] == gr.FX_NONE and len(r.chosen) == 64
        assert np.array_equal(np.unique(r.position), heads)
    finally:
        dev.close(); host.close()


def test_samples_panel_device_equals_host_and_the_cap_is_refused():
    p, want = refs.samples_panel()
    dev, host = _both(p, np.arange(p.n_groups))
    try:
        r = _agree(dev, host, gr.SIGNED, None, (), 25)
        assert r.n_samples.tolist() == want and dev.timing["n_long"] == 6
    finally:
        dev.close(); host.close()
    big, _ = refs.samples_panel(65538)  # ids up to the cap + 1
    for engine in ("device", "host"):
        with pytest.raises(_lib.HawkStatusError) as e:
            gr.GroupEffects(big, big.hap_samples, big.is_ref_hap, np.arange(big.n_groups), engine).rank(gr.SIGNED, None, (), 25)
        assert e.value.status == _lib.HAWK_E_UNSUPPORTED


def test_rule_panels_ties_and_zero_groups_device_equals_host():
    p = refs.rules_panel()
    for order in (np.arange(p.n_groups), np.arange(p.n_groups)[::-1].copy()):
        dev, host = _both(p, order)
        r = _agree(dev, host, gr.SIGNED, None, (), 25)
        assert r.type.tolist() == [0, 2, 2, 3, 0, 3, 1, 0, 255] and int(r.dup.sum()) == 1
        _agree(dev, host, gr.ABSOLUTE, np.array([0.5, np.nan, 0.9, 0.1, 0.5, 0.6, 0.3, np.nan, 0.2]), (), 25)
        dev.close(); host.close()
    pr = refs.right_panel()
    dev, host = _both(pr, np.arange(3))
    assert _agree(dev, host, gr.SIGNED, None, (), 1).type.tolist() == [0, 3, 2]
    dev.close(); host.close()
    p, order = refs.tie_panel()   # K = 25 over 30 tied positions, and K = 25 with 24 positions
    dev, host = _both(p, order)
    r = _agree(dev, host, gr.SIGNED, None, (), 25)
    assert r.pos_first_rank[r.chosen].tolist() == sorted(r.pos_first_rank[r.position == np.arange(p.n_groups)].tolist())[:25]
    dev.close(); host.close()
    p24, order24 = refs.tie_panel(24)
    dev, host = _both(p24, order24)
    assert len(_agree(dev, host, gr.SIGNED, None, (), 25).chosen) == 24
    dev.close(); host.close()
    empty = refs.Panel().build()
    dev, host = _both(empty, np.zeros(0, np.int64))
    r = _agree(dev, host, gr.SIGNED, None, (), 25)
    assert len(r.chosen) == 0 and r.alt_off.tolist() == [0]
    dev.close(); host.close()


def test_search_files_writes_delta_type_and_candidate_tables(tmp_path):
    """FASTA + BED + VCF -> pipeline.search_files(graphical_reports=True, candidate_guides=[...]): the delta table equals the
    reference's under the comparison rule, the type counts and the candidates' sub-reports equal the fixture's text; a tiled
    search refuses the stage"""
    import pandas as pd
    from crisprhawk_hip import pipeline, readers, tiling
    from util import load_golden
    name = "phased4"
    fx = load_golden(f"g7_report_{name}.json.gz")
    rec = refs.g14()["fixtures"][name]
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf.gz")
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts] for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, True)
    cstr = [f"{fx['contig']}:{g.split('_')[-2]}:{g.split('_')[-1]}" for g in rec["candidates"]["two"]]
    figures = {}
    paths = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=synth.cfd_tables(),
                                  graphical_reports=True, candidate_guides=cstr, figures=figures)
    (path,) = paths.values()
    assert open(path).read() == fx["report_tsv"]
    (made,) = figures.values()
    base = {os.path.basename(p): p for p in made}
    prefix = f"{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}"
    subs = {f"crisprhawk_candidate_guides__{fx['contig']}_{c.split(':')[1]}_{fx['pam']}_{fx['guidelen']}.tsv" for c in cstr}
    assert set(base) == {f"{prefix}_score_cfdon_delta.tsv", f"{prefix}_guides_type.tsv"} | subs and len(subs) == 2
    assert os.path.basename(os.path.dirname(base[f"{prefix}_guides_type.tsv"])) == "figures"
    df = pd.read_csv(base[f"{prefix}_score_cfdon_delta.tsv"], sep="\t", float_precision="round_trip")  # (to_csv prints doubles so that they read back exactly)
    refs.compare_table(df, rec["tables"]["cfdon_two"], 2, fx["report_tsv"])
    assert "\tNA\t" in open(base[f"{prefix}_score_cfdon_delta.tsv"]).read() or rec["tables"]["cfdon_two"]["max_alts"] == 1
    counts = dict(l.split("\t") for l in open(base[f"{prefix}_guides_type.tsv"]).read().splitlines()[1:])
    assert {k: int(v) for k, v in counts.items()} == rec["type_counts"]
    for k in subs:
        assert open(base[k]).read() == rec["subreports"][k]
    with pytest.raises(ValueError, match="graphical_reports"):
        tiling.TiledRegionSearch.run(None, graphical_reports=True)


def test_search_files_with_a_model_scorer_runs_the_stage_on_the_flanked_collapse(tmp_path):
    """DeepCpf1 on (Cpf1, right=True): the collapse runs with flank (4, 3), so groups may differ in the flanks only - the type
    counts must be those of the report's distinct guides (drop_duplicates on the extended guide id, then the type rule), and the
    delta table of score_deepcpf1 must be the absolute family's on the report's own printed scores"""
    import pandas as pd
    from crisprhawk_hip import pipeline, readers
    from util import load_golden
    fx = load_golden("g7_report_cpf1.json.gz")
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], contig_seq, 80)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts] for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    figures = {}
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"),
                                    deepcpf1_weights=synth.deepcpf1_weights(), graphical_reports=True, figures=figures).values()
    (made,) = figures.values()
    base = {os.path.basename(p): p for p in made}
    prefix = f"{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}"
    assert set(base) == {f"{prefix}_score_deepcpf1_delta.tsv", f"{prefix}_guides_type.tsv"}
    rep = pd.read_csv(path, sep="\t", float_precision="round_trip")
    low = lambda s: any(c.islower() for c in s)
    uniq = rep.drop_duplicates(subset=["chr", "start", "stop", "strand", "sgRNA_sequence", "pam"])
    want = {label: 0 for label in gr.GUIDETYPES.values()}
    for o, sg, pm in zip(uniq["origin"], uniq["sgRNA_sequence"], uniq["pam"]):
        want[gr.GUIDETYPES[0 if o == "ref" else 1 if low(sg) and low(pm) else 2 if low(sg) else 3]] += 1
    counts = dict(l.split("\t") for l in open(base[f"{prefix}_guides_type.tsv"]).read().splitlines()[1:])
    assert {k: int(v) for k, v in counts.items()} == want and len(uniq) <= len(rep)
    # the delta table: per position |score - ref score| of every alternative, worst = Python's max over them in report order
    df = pd.read_csv(base[f"{prefix}_score_deepcpf1_delta.tsv"], sep="\t", float_precision="round_trip")
    rep["gid"] = rep["chr"] + "_" + rep["start"].astype(str) + "_" + rep["strand"]
    worst = {}
    for gid, grp in rep.groupby("gid", sort=False):
        ref = grp[grp["origin"] == "ref"]
        if len(ref):
            d = [abs(x - ref["score_deepcpf1"].values[0]) for x in grp[grp["origin"] == "alt"]["score_deepcpf1"].tolist()]
            worst[gid] = max(d) if d else 0.0
    first = {g: i for i, g in reversed(list(enumerate(rep["gid"])))}
    ranked = sorted(worst, key=lambda g: (-worst[g], first[g]))[:25]
    assert df["guide_id"].tolist() == ranked and df["Rank"].tolist() == list(range(1, len(ranked) + 1))
    for gid, a1 in zip(df["guide_id"], df["alt1_abs_delta"]):
        if worst[gid] > 0:
            assert a1 == a1 and a1 <= worst[gid]
