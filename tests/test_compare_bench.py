"""tools/compare_bench.py, the one definition of the comparison tools' measurement protocol, against every record those tools have
committed under profiles/: the module's stats() and verdict() give back the stored spread, ratio and verdict bit for bit.  A record keeps
[min, median, max] of a side's rounds; the median, the extrema and so the spread and the verdict of that triple are those of the rounds.
No GPU: the module imports torch only inside the functions that time."""
import argparse
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("compare_bench", os.path.join(ROOT, "tools", "compare_bench.py"))
cb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cb)

PROFILES = ("attention_dropout", "attention_edge", "edge_dot", "edge_op", "gat_attention", "gat_attention_u_sweep", "gatv2_attention",
            "score_attention", "score_attention_passes", "spmm_edge", "spmm_edge_multi", "spmm_edge_softagg", "spmm_gated", "spmm_multi",
            "spmm_reduce", "spmm_softagg", "vector_attention")
STATS_KEYS = {"median_us", "min_us", "max_us", "spread"}
DROPOUT_WORDS = {"plain": "costs", "dropout": "faster", "undecided": "within_spread"}   # tools/attention_dropout_bench.py


def is_stats(x):
    return isinstance(x, dict) and STATS_KEYS <= set(x)


def triple(block):
    return [block["min_us"], block["median_us"], block["max_us"]]


def blocks(x):
    """every dict of a record, the record itself included"""
    if isinstance(x, dict):
        yield x
        for v in x.values():
            yield from blocks(v)


def records():
    for name in PROFILES:
        with open(os.path.join(ROOT, "profiles", name + ".jsonl")) as fh:
            for line in fh:
                yield name, json.loads(line)


def test_every_committed_stats_block_is_stats_of_its_triple():
    n = 0
    for name, rec in records():
        for b in blocks(rec):
            if is_stats(b):
                got = cb.stats(triple(b))
                assert {k: got[k] for k in STATS_KEYS} == {k: b[k] for k in STATS_KEYS}, (name, b)
                n += 1
    assert n == 1140


def test_every_committed_verdict_is_verdict_of_its_two_sides():
    """256 blocks with a "fused" and a "composition" side; besides them every other block of these files that holds a verdict:
    60 of score_attention ("fused" against a named side, both in the block), 50 of edge_dot and 20 of spmm_edge (the verdict on the
    baseline's own block, the subject's block beside it in the same pass), 60 + 12 of attention_dropout (plain against dropout in the
    tool's words; the dropout entry, stored as "dropout", against the composition).  No block with a verdict is left out: the last
    assertion counts them all."""
    n = {"fused_composition": 0, "score_attention": 0, "edge_dot": 0, "spmm_edge": 0, "dropout_price": 0, "dropout_composition": 0}
    verdicts = 0
    for name, rec in records():
        verdicts += sum("verdict" in b for b in blocks(rec))
        for b in blocks(rec):
            sides = [k for k, v in b.items() if is_stats(v)]
            if "verdict" in b and "fused" in sides and "composition" in sides:
                assert cb.verdict(triple(b["fused"]), triple(b["composition"]), "fused", "composition") == (b["ratio"], b["verdict"]), (name, b)
                n["fused_composition"] += 1
            elif "verdict" in b and name == "score_attention":
                (other,) = [s for s in sides if s != "fused"]
                assert cb.verdict(triple(b["fused"]), triple(b[other]), "fused", other) == (b["ratio"], b["verdict"]), (name, b)
                n[name] += 1
            elif "verdict" in b and name == "attention_dropout" and "plain" in sides:
                ratio, v = cb.verdict(triple(b["plain"]), triple(b["dropout"]), "plain", "dropout")
                assert (ratio, DROPOUT_WORDS[v]) == (b["ratio"], b["verdict"]), (name, b)
                n["dropout_price"] += 1
            elif "verdict" in b and name == "attention_dropout":
                assert cb.verdict(triple(b["dropout"]), triple(b["composition"]), "fused", "composition") == (b["ratio"], b["verdict"]), (name, b)
                n["dropout_composition"] += 1
            subject = {"edge_dot": "edge_dot", "spmm_edge": "fused"}.get(name)
            if subject in sides:   # a pass of a named-baseline record: the subject's block, the baselines' blocks beside it
                for other, c in b.items():
                    if other != subject and is_stats(c):
                        other_name = other if name == "edge_dot" else "composition"
                        assert cb.verdict(triple(b[subject]), triple(c), subject, other_name) == (c["ratio"], c["verdict"]), (name, other, c)
                        assert cb.baseline_block(triple(b[subject]), triple(c), subject, other_name) == c, (name, other, c)
                        n[name] += 1
    assert n == {"fused_composition": 256, "score_attention": 60, "edge_dot": 50, "spmm_edge": 20, "dropout_price": 60, "dropout_composition": 12}
    assert verdicts == sum(n.values())


def test_two_sided_block_has_the_committed_key_order():
    with open(os.path.join(ROOT, "profiles", "gat_attention.jsonl")) as fh:
        b = json.loads(fh.readline())["forward"]
    got = cb.two_sided(triple(b["fused"]), triple(b["composition"]))
    assert list(got) == [k for k in b if k != "reps"] and got == {k: v for k, v in b.items() if k != "reps"}


@pytest.mark.parametrize("once_us, want", [(1e9, 1), (50_000.0, 4), (60_000.0, 3), (10.0, 8)])
def test_choose_reps(once_us, want):
    """a call longer than the round: 1; in between: round / call, rounded down; a short call: max_reps"""
    assert cb.choose_reps(once_us, 200.0, 8) == want
    assert isinstance(cb.choose_reps(once_us, 200.0, 8), int)


def test_protocol_args_have_todays_defaults():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    assert vars(ap.parse_args([])) == {"matrix": "small", "rounds": 5, "round_ms": 200.0, "max_reps": 8, "tag": "", "out": ""}
    for m in ("config4", "fem", "powerlaw", "small"):
        assert ap.parse_args(["--matrix", m]).matrix == m
    with pytest.raises(SystemExit):
        ap.parse_args(["--matrix", "other"])
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap, tag=False)
    assert "tag" not in vars(ap.parse_args([]))


def test_emit_appends_one_line_and_creates_the_directory(tmp_path, capsys):
    out = tmp_path / "new" / "dir" / "x.jsonl"
    cb.emit({"b": 1, "a": {"c": 2.5}}, str(out))
    cb.emit({"z": 0}, str(out))
    assert out.read_text() == '{"b": 1, "a": {"c": 2.5}}\n{"z": 0}\n'
    assert capsys.readouterr().out == out.read_text()
    cb.emit({"z": 0}, "")   # no file asked for: the line alone
    assert capsys.readouterr().out == '{"z": 0}\n' and len(list(tmp_path.iterdir())) == 1


def test_diff_sees_a_moved_key_and_a_changed_value_and_no_timing(tmp_path):
    a = {"matrix": "small", "M": 3, "forward": {"fused": {"median_us": 1.0, "min_us": 1.0, "max_us": 1.0, "spread": 0.0}, "reps": 2}}
    same = json.loads(json.dumps(a)); same["forward"]["fused"]["median_us"] = 9.0; same["forward"]["reps"] = 5
    moved = {"M": 3, "matrix": "small", "forward": a["forward"]}
    changed = dict(a, M=4)
    for n, rec in (("a", a), ("same", same), ("moved", moved), ("changed", changed)):
        (tmp_path / n).write_text(json.dumps(rec) + "\n")
    assert cb.diff(str(tmp_path / "a"), str(tmp_path / "same")) == 0
    assert cb.diff(str(tmp_path / "a"), str(tmp_path / "moved")) == 1
    assert cb.diff(str(tmp_path / "a"), str(tmp_path / "changed")) == 1
