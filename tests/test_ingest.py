"""Ingest codec: CPU checks of the oracle and of the device parser.

The device record parser (spatialflink_amd/csrc/ingest_parse.h) is __host__ __device__ code;
``_abi.debug_ingest_record`` runs the same functions host-compiled, so these tests check its
decisions without a GPU.  The kernels that split a batch into records and run the parser per
lane are checked on the GPU by tests/test_gpu_ingest.py, and tests/test_gpu_ingest_numeric.py
runs these same cases through them: the known answers and the fuzz generators live in
tests/ingest_cases.py, shared by both.

Known answers are derived by hand from the Java code (paths relative to
/root/reference/src/main/java/GeoFlink): CSVTSVToSpatial / CSVTSVToTSpatial
spatialStreams/Deserialization.java:248-254, 306-321 (quote removal, split on \\s*d\\s*,
Double.valueOf / Long.valueOf); GeoJSONToSpatial :132-146; WKTToSpatial :223-228, :1510-1514.
The reference holds no deserializer fixtures, so parity of the grammar corners is unpinned
beyond these hand-derived answers (Parity).
"""
from __future__ import annotations

import math
import random
import struct
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

import cref  # noqa: E402  (oracle: the checker)
from spatialflink_amd import _abi  # noqa: E402

from ingest_cases import (CSV, KNOWN, TSV, WKT, _rand_decimal, halfway_tokens, halfway_values,  # noqa: E402
                          hex_or_long_exponent_token)

_FMT = {"csv": cref.CSV, "geojson": cref.GEOJSON, "wkt": cref.WKT}


def _spec_oracle(s):
    return cref.ingest_spec(_FMT[s[0]], s[1], s[2], s[3], s[4])


def _spec_dev(s):
    return _abi.make_ingest_spec(_FMT[s[0]], s[1], s[2], s[3], s[4])


def _bits(v):
    return struct.pack("<d", v)


def _same(a, b):
    return _bits(a) == _bits(b) or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("spec,rec,want,may_reject", KNOWN)
def test_oracle_known_answers(spec, rec, want, may_reject):
    got = cref.ingest_record(_spec_oracle(spec), rec)
    if want is None:
        assert got is None
    else:
        assert got is not None and _same(got[0], want[0]) and _same(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("spec,rec,want,may_reject", KNOWN)
def test_device_parser_known_answers(spec, rec, want, may_reject):
    got = _abi.debug_ingest_record(_spec_dev(spec), rec)
    if want is None:
        assert got is None
    elif got is None:
        assert may_reject, "device parser rejected a record it must decide"
    else:
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and got[2] == want[2]


def test_decimal_conversion_fuzz():
    """Random decimal tokens: device parser == oracle == Python float (all correctly rounded)."""
    rng = random.Random(20260116)
    spec_d, spec_o = _spec_dev(TSV), _spec_oracle(TSV)
    rejected = 0
    n = 20000
    for _ in range(n):
        a, b = _rand_decimal(rng), _rand_decimal(rng)
        rec = f"{a}\t{b}".encode()
        want = (float(a), float(b))
        o = cref.ingest_record(spec_o, rec)
        assert o is not None and _same(o[0], want[0]) and _same(o[1], want[1]), rec
        d = _abi.debug_ingest_record(spec_d, rec)
        if d is None:
            rejected += 1
            sig = [len(t.lstrip("+-").split("e")[0].split("E")[0].replace(".", "").lstrip("0")) for t in (a, b)]
            assert max(sig) > 19, f"rejected a token of <= 19 significant digits: {rec}"
            continue
        assert _same(d[0], want[0]) and _same(d[1], want[1]), rec
    assert rejected < n // 100


def test_decimal_halfway_cases():
    """Points at (and 1e-35 relative around) the midpoint of adjacent doubles, written with 17-41
    significant digits: where the device parser decides, it matches Python's correctly rounded float."""
    spec_d = _spec_dev(TSV)
    vals = halfway_values()
    decided = 0
    for s, digits in halfway_tokens(vals):
        d = _abi.debug_ingest_record(spec_d, f"{s}\t1".encode())
        if d is not None:
            decided += 1
            assert _same(d[0], float(s)), s
        else:
            assert digits + 1 > 19, s
    assert decided > len(vals) * 6


def _noise(rng, chars=" \t\""):
    return "".join(rng.choice(chars) for _ in range(rng.choice([0, 0, 0, 1, 2])))


def test_csv_shape_fuzz():
    """Random spaces, tabs, quotes and control characters around fields: the device parser either
    agrees bit-exactly with the oracle or rejects; it never accepts what the reference rejects."""
    rng = random.Random(99)
    for delim in (",", ";", "\t", " "):
        spec = ("csv", delim, 2, 3, 1)
        sd, so = _spec_dev(spec), _spec_oracle(spec)
        accepted = 0
        for _ in range(4000):
            nf = rng.choice([3, 4, 4, 4, 5])
            fields = []
            for f in range(nf):
                v = rng.choice(["12", "-7", "+3", "1.5", "116.4148990000001", "x", "", "1e5", "0.30000000000000004",
                                "NaN", "2.5d", "1 2", "16\x01"]) if f else rng.choice(["a", "7", "", " q"])
                fields.append(_noise(rng) + v + _noise(rng))
            sep = [rng.choice([delim, " " + delim, delim + " ", '"' + delim + '"', delim + delim])
                   for _ in range(nf - 1)]
            rec = fields[0] + "".join(s + f for s, f in zip(sep, fields[1:]))
            rec = rec.encode()
            o = cref.ingest_record(so, rec)
            d = _abi.debug_ingest_record(sd, rec)
            if o is None:
                assert d is None, (delim, rec, d)
            elif d is not None:
                accepted += 1
                assert _same(d[0], o[0]) and _same(d[1], o[1]) and d[2] == o[2], (delim, rec, d, o)
        assert accepted > 200, delim


def test_oracle_batch_framing():
    spec = _spec_oracle(CSV)
    one = cref.ingest(spec, b"a,b,1,2")
    assert one["x"].tolist() == [1.0]
    two = cref.ingest(spec, b"a,b,1,2\na,b,3,4\n")  # a trailing '\n' ends the last record
    assert two["y"].tolist() == [2.0, 4.0]
    assert len(cref.ingest(spec, b"")["x"]) == 0
    with pytest.raises(cref.IngestRejected) as e:
        cref.ingest(spec, b"a,b,1,2\n\na,b,3,4")  # an empty line is a record: get(2) throws
    assert e.value.bad == 1


def test_oracle_cell_assignment():
    """Point(x, y, uGrid) -> HelperClass.assignGridCellID (HelperClass.java:104-116)."""
    g = cref.grid(115.5, 39.6, (117.6 - 115.5) / 100, 100)
    got = cref.ingest_record(_spec_oracle(WKT), b"POINT (116.414899 39.920374)", g)
    cx, cy = cref.cell(g, 116.414899, 39.920374)
    assert (cx, cy) == (43, 15)  # the README query cell
    assert got[3] == 43 * 100 + 15
    assert cref.ingest_record(_spec_oracle(WKT), b"POINT (117.6 39.7)", g)[3] == 0xFFFFFFFF  # cx == n
    assert cref.ingest_record(_spec_oracle(WKT), b"POINT (NaN 39.7)", g)[3] == 0 * 100 + 4  # (int)NaN == 0


def test_spec_validation():
    with pytest.raises(_abi.GeohipArgumentError):
        _abi.debug_ingest_record(_abi.make_ingest_spec(cref.CSV, "|", 0, 1), b"1|2")  # regex metacharacter
    with pytest.raises(_abi.GeohipArgumentError):
        _abi.debug_ingest_record(_abi.make_ingest_spec(cref.CSV, ",", -1, 1), b"1,2")


def test_hex_and_long_exponent_fuzz():
    """Random hex significands (Double.parseDouble's parseHexString grammar) and decimal tokens with
    long exponents: device parser == oracle (glibc strtod, correctly rounded) == Python."""
    rng = random.Random(424242)
    spec_d, spec_o = _spec_dev(TSV), _spec_oracle(TSV)
    for _ in range(20000):
        toks = [hex_or_long_exponent_token(rng), hex_or_long_exponent_token(rng)]
        rec = f"{toks[0][0]}\t{toks[1][0]}".encode()
        o = cref.ingest_record(spec_o, rec)
        d = _abi.debug_ingest_record(spec_d, rec)
        assert o is not None and d is not None, rec
        for k in range(2):
            assert _same(o[k], toks[k][1]) and _same(d[k], toks[k][1]), (rec, o, d)
