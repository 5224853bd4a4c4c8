"""CPU checks of the corpora that tests/test_gpu_ingest_numeric.py drives through the kernels.

Before a GPU compares anything, the cases themselves are pinned here, without a device:
  * the C oracle (glibc strtod, Java grammar) equals Python ``float()`` bit-for-bit on every token;
  * the host-compiled device parser (``_abi.debug_ingest_record``) either equals both or rejects,
    and it rejects only tokens of more than 19 significant digits;
  * a GPU test cannot hide a failure by leaving cases out: per corpus, the share of records the
    host-compiled parser rejects although the oracle accepts them stays under 1 % (the cap of
    test_ingest.py::test_decimal_conversion_fuzz), and the number corpus (at most 19 significant
    digits per token) loses nothing at all.  The halfway corpus is the one exception the cases
    themselves make: half of its tokens carry 21 or 41 digits around an exact midpoint, which the
    parser rejects by design; the GPU test runs rejected ones for their rejection instead;
  * each record layout takes its conversion site by the kernels' own acceptance rules
    (``ingest_cases.check_layout``), asserted on the text -- nothing measures which path ran.
"""
from __future__ import annotations

import math
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

import cref  # noqa: E402  (oracle: the checker)
from spatialflink_amd import _abi  # noqa: E402

import ingest_cases as C  # noqa: E402


def _same(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (math.isnan(a) and math.isnan(b))


SPEC_O = cref.ingest_spec(cref.CSV, "\t", 0, 1, -1)
SPEC_D = _abi.make_ingest_spec(cref.CSV, "\t", 0, 1, -1)


def _token_pairs_check(pairs, cap_share=0.01):
    """pairs: [((tok, want), (tok, want))].  Returns the number of records the host parser rejects."""
    rejected = 0
    for (a, wa), (b, wb) in pairs:
        rec = f"{a}\t{b}".encode()
        o = cref.ingest_record(SPEC_O, rec)
        assert o is not None and _same(o[0], wa) and _same(o[1], wb), rec[:80]
        d = _abi.debug_ingest_record(SPEC_D, rec)
        if d is None:
            rejected += 1
            assert max(C.sig_digits(a), C.sig_digits(b)) > 19, f"rejected <= 19 significant digits: {rec[:80]}"
            continue
        assert _same(d[0], wa) and _same(d[1], wb), rec[:80]
    assert rejected < cap_share * len(pairs), (rejected, len(pairs))
    return rejected


def test_number_corpus_tokens():
    corpus = C.number_corpus()
    classes = {k: sum(1 for c, _ in corpus if c == k) for k in "abcde"}
    assert 20000 <= len(corpus) <= 40000 and all(classes[k] > 300 for k in "abcde"), classes
    splits = {(len(t.split(".")[0]), len(t.split(".")[1]) if "." in t else 0) for c, t in corpus if c == "a"}
    assert all((ni, nf) in splits for ni in range(1, 20) for nf in range(0, 20 - ni))
    rejected = _token_pairs_check([((t, float(t)), ("1", 1.0)) for _, t in corpus])
    assert rejected == 0  # at most 19 significant digits: nothing may be left out
    want = np.array([float(t) for _, t in corpus])
    # the corpus lands where the issue asks: ties, subnormals, the normal edge, underflow, -0
    assert np.sum((want != 0) & (np.abs(want) < 2.2250738585072014e-308)) > 100
    assert np.sum((want == 0) & np.array([C.sig_digits(t) > 0 for _, t in corpus])) > 20
    assert float("0." + "0" * 323 + "2470328229206232720") == 0.0
    assert float("0." + "0" * 323 + "2470328229206232721") == 5e-324
    assert sum(1 for _, t in corpus if not C.swar_takes(t)) > 2000  # left out of the first layout


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("kind", ["swar", "fast", "general"])
def test_layouts_force_their_path(kind, swap):
    text, rows, xt, yt = C.layout(kind, swap)
    assert len(text) < 4.5e6
    C.check_layout(kind, text, rows)
    o = cref.ingest(cref.ingest_spec(cref.CSV, ",", 2, 3, 1), text)
    assert np.array_equal(o["x"][rows].view(np.uint64), np.array([float(t) for t in xt]).view(np.uint64))
    assert np.array_equal(o["y"][rows].view(np.uint64), np.array([float(t) for t in yt]).view(np.uint64))
    if kind == "general" and not swap:  # the host-compiled parser on the very records
        sd = _abi.make_ingest_spec(cref.CSV, ",", 2, 3, 1)
        for r, rec in enumerate(text.split(b"\n")[:-1]):
            d = _abi.debug_ingest_record(sd, rec)
            assert d is not None and _same(d[0], o["x"][r]) and _same(d[1], o["y"][r]) and d[2] == o["ts"][r], rec


def test_general_grammar_corpora():
    _token_pairs_check([((a, float(a)), (b, float(b))) for a, b in C.decimal_fuzz_pairs(10000)])
    assert _token_pairs_check(C.hex_fuzz_pairs(10000)) == 0
    assert _token_pairs_check([(t, ("1", 1.0)) for t in C.special_tokens()]) == 0
    _token_pairs_check(C.large_value_batch())
    rej = [t for t, w in C.large_value_tokens() if _abi.debug_ingest_record(SPEC_D, f"{t}\t1".encode()) is None]
    # half an ulp above DBL_MAX lies between the 19-digit truncation's two candidates: the one
    # large token the parser may hand to the host
    assert all(len(t) > 300 for t in rej) and len(rej) <= 2, [t[:30] for t in rej]
    want = dict(C.large_value_tokens())
    dbl_max = int(float.fromhex("0x1.fffffffffffffp1023"))
    assert want[str(dbl_max)] == 1.7976931348623157e308 and want[str(dbl_max + (1 << 970))] == math.inf
    assert want[str(dbl_max + (1 << 970) - 1)] == 1.7976931348623157e308


def test_halfway_corpus_split():
    """Halfway tokens: decided ones equal float(); the rest carry more than 19 digits."""
    toks = C.halfway_tokens()
    decided = rejected = 0
    for s, digits in toks:
        o = cref.ingest_record(SPEC_O, f"{s}\t1".encode())
        assert o is not None and _same(o[0], float(s)), s
        d = _abi.debug_ingest_record(SPEC_D, f"{s}\t1".encode())
        if d is None:
            rejected += 1
            assert digits + 1 > 19
        else:
            decided += 1
            assert _same(d[0], float(s)), s
    assert decided >= len(toks) // 2 and rejected >= 32


@pytest.mark.parametrize("off", [-720, 0, 330, 840])
def test_trajectory_dates(off):
    """The lenient dates of the GPU test: host-compiled parser == oracle == Python's calendar."""
    sd, td = _abi.make_ingest_spec(cref.GEOJSON), _abi.make_traj_spec(utc_offset_min=off)
    dates = C.date_strings() + list(C.DATE_ZERO)
    text = b"\n".join(C.date_record(s, i) for i, s in enumerate(dates))
    want = cref.ingest_traj(cref.ingest_spec(cref.GEOJSON), cref.traj_spec(utc_offset_min=off), text)["ts"]
    known = 0
    for i, s in enumerate(dates):
        d = _abi.debug_ingest_traj_record(sd, td, C.date_record(s, i))
        assert d is not None and d[2] == want[i], s
        if s in C.DATE_ZERO:
            assert d[2] == 0
        elif C.date_millis(s, off) is not None:
            known += 1
            assert d[2] == C.date_millis(s, off), s
    assert known > 0.9 * len(dates)
    for s in C.DATE_CONTROL:  # also in another string value and in a key
        for rec in (C.date_record(s, 1), C.date_record("2008-02-02 20:12:32", 1).replace(b'"oID"', b'"k":"' + s.encode()
                                                                                       + b'","oID"'),
                    C.date_record("2008-02-02 20:12:32", 1).replace(b'"oID"', b'"' + s.encode() + b'":1,"oID"')):
            assert _abi.debug_ingest_traj_record(sd, td, rec) is None, rec
            with pytest.raises(cref.IngestRejected):
                cref.ingest_traj(cref.ingest_spec(cref.GEOJSON), cref.traj_spec(utc_offset_min=off), rec)


def test_trajectory_long_timestamps():
    sd, so = _abi.make_ingest_spec(cref.CSV, ",", 2, 3, 1, 0), cref.ingest_spec(cref.CSV, ",", 2, 3, 1, 0)
    for t in C.LONG_OK:
        rec = f"v,{t},116.5,39.75".encode()
        assert _abi.debug_ingest_traj_record(sd, None, rec)[2] == int(t) == cref.ingest_traj(so, None, rec)["ts"][0]
    for t in C.LONG_BAD:
        rec = f"v,{t},116.5,39.75".encode()
        assert _abi.debug_ingest_traj_record(sd, None, rec) is None
        with pytest.raises(cref.IngestRejected):
            cref.ingest_traj(so, None, rec)


def test_geometry_batches():
    """The chunk-geometry batches are what their tests say: record counts per chunk, sweep offsets."""
    counts = C.chunk_record_counts(C.fixed_records(6, 50000))
    assert counts[0] == C.FAST_STARTS + 1 and (counts[1:-1] == C.FAST_STARTS).all()
    for length, rounds in ((7, 7), (8, 6), (12, 4), (24, 2)):
        full = C.chunk_record_counts(C.fixed_records(length, 30000))[1:-1]
        assert {-(-int(c) // C.THREADS) for c in full} == {rounds}
    assert (C.chunk_record_counts(C.fixed_records(5, 50000))[1:-1] > C.FAST_STARTS).all()
    so = cref.ingest_spec(cref.CSV, ",", 2, 3, 1)
    for pad in (0, 700):
        text, rows, xt, yt = C.boundary_sweep(pad)
        assert len(text) < 4_000_000 and len(rows) == 133
        o = cref.ingest(so, text)
        assert np.array_equal(o["x"][rows].view(np.uint64), np.array([float(t) for t in xt]).view(np.uint64))
    n = 0
    for text, row, a, b in C.batch_end_sweep():
        o = cref.ingest(so, text)
        assert o["x"][row] == float(a) and o["y"][row] == float(b)
        n += 1
    assert n == 125


def test_cell_and_special_batches_parse_on_the_host():
    """Every record of the extreme-coordinate and special-token batches is inside the device grammar."""
    for mn in (115.5, -1.0):
        toks = C.cell_axis_values(mn, 0.02, 100)
        assert len(toks) == 7 + 7 * 7
        for spec, fmt in (((cref.WKT,), "POINT ({a} {b})"), ((cref.CSV, ",", 2, 3, 1), "1,2,{a},{b}")):
            for a, b in zip(toks, toks[5:] + toks[:5]):
                rec = fmt.format(a=a, b=b).encode()
                d = _abi.debug_ingest_record(_abi.make_ingest_spec(*spec), rec)
                o = cref.ingest_record(cref.ingest_spec(*spec), rec)
                assert d is not None and o is not None and _same(d[0], o[0]) and _same(d[1], o[1]), rec
                assert _same(d[0], float(a)) and _same(d[1], float(b)), rec
    sp = C.special_tokens()
    for spec, fmt in (((cref.WKT,), "POINT ({a} {b})"), ((cref.CSV, ",", 2, 3, 1), "1,2,{a},{b}")):
        for a, b in zip(sp, sp[11:] + sp[:11]):
            rec = fmt.format(a=a[0], b=b[0]).encode()
            d = _abi.debug_ingest_record(_abi.make_ingest_spec(*spec), rec)
            o = cref.ingest_record(cref.ingest_spec(*spec), rec)
            assert d is not None and o is not None, rec
            assert _same(d[0], o[0]) and _same(d[0], a[1]) and _same(d[1], o[1]) and _same(d[1], b[1]), rec
