"""GPU: the ingest codec's number conversion over the whole double range, its general grammar,
its cells of extreme coordinates and its chunk geometry, as compiled for gfx950.

tests/test_ingest.py checks the record grammar (csrc/ingest_parse.h) host-compiled only.  The
kernels (csrc/ingest.hip) run it compiled for the device -- decimal_to_bits through __umul64hi
and the __device__ copy of kPow5 -- and add two conversion sites that exist only there: swar_csv
(digit values from udot4 / umul24 sums) and fast_csv.  This file drives the same cases
(tests/ingest_cases.py) through the kernels.

References: a number token's value is Python float(token) / float.fromhex (correctly rounded);
a record's (x, y, ts, cell) is the C oracle's (glibc strtod, Java grammar).  Values compare by
bits (NaN equal to NaN), timestamps and cells exactly.  tests/test_ingest_corpus.py pins the
corpora on the CPU first: oracle == float(), the host-compiled parser equals both or rejects only
tokens of more than 19 significant digits, and under 1 % of a corpus is left out here for that.

Which conversion site a record takes follows from the kernels' own acceptance rules, by
construction of the text (ingest_cases.check_layout asserts them on the text); nothing here
measures which path ran.
  swar    'id,ts,x,y', short fields: every field ends inside its 24-byte window (ingest.hip:289,
          296, 316), at most 19 digits counting leading zeros (:301), field starts within 72 bytes
          (:280), 112 staged bytes after the record start (:273) -> swar_csv decides (:439).
  fast    a 30-character objID: field 0 has no stop byte in its window, so swar_csv returns kSwarNo
          (:313-316) and fast_csv runs (:440); it takes any count of leading zeros and fraction
          digits with at most 19 significant ones (:138-141), the record inside the staged bytes
          (:151, :168).  Carries the long fractions and the long-leading-zero tokens.
  general one quoted or blank-padded record per chunk: fast_csv stops at '"' / ' ' (:166, :180),
          the chunk is listed (:462-467) and ingest_general re-parses every record of it with
          parse_record (:490-499).  A whitespace delimiter or a GeoJSON / WKT batch sends every
          chunk there (:424-425, :437-442).
"""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

import cref  # noqa: E402  (oracle: the checker)
from spatialflink_amd import _abi, synth  # noqa: E402

import ingest_cases as C  # noqa: E402
# chunk geometry, written once in ingest_cases.py: csrc/ingest.h:20-21, csrc/ingest.hip:339
from ingest_cases import CHUNK, FAST_STARTS, TAIL, THREADS  # noqa: E402

pytestmark = pytest.mark.gpu

BJ = synth.BEIJING
GRIDS = {"beijing": (BJ[0], BJ[2], (BJ[1] - BJ[0]) / 100, 100), "unit": (-1.0, -1.0, 0.02, 100)}
_FMT = {"csv": cref.CSV, "geojson": cref.GEOJSON, "wkt": cref.WKT}


def _specs(s):
    return (_abi.make_ingest_spec(_FMT[s[0]], s[1], s[2], s[3], s[4]),
            cref.ingest_spec(_FMT[s[0]], s[1], s[2], s[3], s[4]))


def _floats(toks):
    return np.array([float(t) for t in toks])


def _assert_bits(got, want, what, labels=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i}: got {got[i]!r} "
                             f"({got.view(np.uint64)[i]:#x}), want {want[i]!r} ({want.view(np.uint64)[i]:#x})"
                             + (f", token {labels[i][:60]!r}" if labels is not None else ""))


def _device_text(text: bytes):
    import torch
    return torch.frombuffer(bytearray(text) or bytearray(1), dtype=torch.uint8)[:len(text)].to("cuda:0")


def _ingest(ctx, spec, text: bytes, grid=None, device=False):
    sd, _ = _specs(spec)
    g = _abi.make_grid(*grid) if grid is not None else None
    got = ctx.ingest_points(sd, _device_text(text) if device else text, g, with_ts=spec[4] >= 0,
                            with_cell=grid is not None)
    if device:
        got = {k: v.cpu().numpy() for k, v in got.items()}
    return got


def _oracle(spec, text: bytes, grid=None):
    return cref.ingest(_specs(spec)[1], text, cref.grid(*grid) if grid is not None else None)


def _assert_oracle(got, want, spec, cell=False):
    assert len(got["x"]) == len(want["x"])
    _assert_bits(got["x"], want["x"], "x against the oracle")
    _assert_bits(got["y"], want["y"], "y against the oracle")
    if spec[4] >= 0:
        assert np.array_equal(got["ts"], want["ts"])
    if cell:
        assert np.array_equal(got["cell"].view(np.uint32), want["cell"])


def _assert_rejects_at(ctx, spec, lines, bad_at):
    """The batch call names record bad_at, as the oracle does where the reference throws."""
    text = b"\n".join(lines)
    with pytest.raises(_abi.GeohipUnsupportedError) as d:
        ctx.ingest_points(_specs(spec)[0], text, with_ts=spec[4] >= 0)
    assert d.value.bad == bad_at, (d.value.bad, bad_at, lines[bad_at][:80])


def _lone_bad(ctx, spec, rec: bytes, j: int, n=300):
    at = (j * 53 + 7) % n
    lines = [C.ordinary_record(spec, i) for i in range(n)]
    lines[at] = rec
    _assert_rejects_at(ctx, spec, lines, at)
    return lines, at


# ---- 1. one number corpus through each of the three conversion sites -----------------------------

@functools.lru_cache(maxsize=None)
def _layout_case(kind, swap):
    text, rows, xt, yt = C.layout(kind, swap)
    C.check_layout(kind, text, rows)
    want = _oracle(C.CSV_T, text)
    ts = np.array([C._ts_of(i) for i in range(len(rows))], dtype=np.int64)
    return text, rows, xt, yt, _floats(xt), _floats(yt), ts, want


def _check_layout_run(ctx, kind, swap, device):
    text, rows, xt, yt, fx, fy, ts, want = _layout_case(kind, swap)
    got = _ingest(ctx, C.CSV_T, text, device=device)
    _assert_oracle(got, want, C.CSV_T)
    _assert_bits(got["x"][rows], fx, f"{kind}: x against float()", xt)
    _assert_bits(got["y"][rows], fy, f"{kind}: y against float()", yt)
    assert np.array_equal(got["ts"][rows], ts)


@pytest.mark.parametrize("swap", [False, True], ids=["xy", "yx"])
@pytest.mark.parametrize("kind", ["swar", "fast", "general"])
def test_number_corpus(ctx, kind, swap):
    """Digit splits, ties, neighbours of powers of two and ten, long fractions down to underflow and
    signs (26 k tokens of at most 19 significant digits) through swar_csv, fast_csv and the
    general parser, each token in both number columns."""
    _check_layout_run(ctx, kind, swap, device=False)


def test_number_corpus_device_text(ctx):
    _check_layout_run(ctx, "fast", False, device=True)


# ---- 2. the general grammar on the device ---------------------------------------------------------

def _pairs_batch(ctx, pairs, min_kept=0.99):
    """[((tok, want), (tok, want))] as one TSV batch (every chunk to ingest_general): records the
    host-compiled parser rejects are dropped (under 1 %) and returned."""
    sd = _specs(C.TSV)[0]
    keep, dropped = [], []
    for p in pairs:
        rec = f"{p[0][0]}\t{p[1][0]}".encode()
        (keep if _abi.debug_ingest_record(sd, rec) is not None else dropped).append((rec, p))
    assert len(keep) >= min_kept * len(pairs)
    text = b"\n".join(r for r, _ in keep)
    got = _ingest(ctx, C.TSV, text)
    _assert_oracle(got, _oracle(C.TSV, text), C.TSV)
    _assert_bits(got["x"], [p[0][1] for _, p in keep], "x against Python", [p[0][0] for _, p in keep])
    _assert_bits(got["y"], [p[1][1] for _, p in keep], "y against Python", [p[1][0] for _, p in keep])
    return [r for r, _ in dropped]


def test_decimal_fuzz(ctx):
    """The tokens of test_ingest.py::test_decimal_conversion_fuzz: exponents e+-{0..350}, up to 42 digits."""
    dropped = _pairs_batch(ctx, [((a, float(a)), (b, float(b))) for a, b in C.decimal_fuzz_pairs(10000)])
    for j, rec in enumerate(dropped[:8]):  # the device makes the host's reject decision too
        _lone_bad(ctx, C.TSV, rec, j)


def test_halfway_tokens(ctx):
    """Midpoints of adjacent doubles written with 17-41 digits: decided ones equal float(); the ones
    the host-compiled parser rejects are rejected on the device, naming the record."""
    sd = _specs(C.TSV)[0]
    toks = [s for s, _ in C.halfway_tokens()]
    ok = [s for s in toks if _abi.debug_ingest_record(sd, f"{s}\t1".encode()) is not None]
    decided = set(ok)
    rejected = [s for s in toks if s not in decided]
    assert len(ok) >= len(toks) // 2 and len(rejected) >= 32
    _pairs_batch(ctx, [((s, float(s)), (t, float(t))) for s, t in zip(ok, ok[1:] + ok[:1])], min_kept=1.0)
    step = len(rejected) // 32
    for j, s in enumerate(rejected[::step][:32]):
        _lone_bad(ctx, C.TSV, f"{s}\t1".encode() if j % 2 else f"1\t{s}".encode(), j, n=60)


def test_large_values(ctx):
    """DBL_MAX in 309 digits, 1e308 / 1e309, 1 and 400 zeros, exponents of 7 and 11 digits, among
    decimal fuzz.  Half an ulp above DBL_MAX (Infinity in Java) lies between the two candidates of
    the 19-digit truncation: the parser hands it to the host, and the device must name it."""
    dropped = _pairs_batch(ctx, C.large_value_batch())
    dbl_max = int(float.fromhex("0x1.fffffffffffffp1023"))
    tie = str(dbl_max + (1 << 970)).encode()
    assert any(tie in r for r in dropped)
    for j, rec in enumerate([tie + b"\t1", b"1\t" + tie, b"-" + tie + b"\t2"]):
        _lone_bad(ctx, C.TSV, rec, j)


def test_hex_nan_suffixes(ctx):
    """Hex significands and long exponents (the hex fuzz generator), NaN, +-Infinity, d/D/f/F
    suffixes, a leading '+', '.5' and '5.'."""
    sp = C.special_tokens()
    pairs = C.hex_fuzz_pairs(8000) + [(a, b) for a, b in zip(sp, sp[7:] + sp[:7])]
    assert _pairs_batch(ctx, pairs, min_kept=1.0) == []
    # the same special tokens in CSV and WKT records
    for spec, fmt in ((C.CSV_T, "{i},{i},{a},{b}"), (C.WKT, "POINT ({a} {b})")):
        use = list(zip(sp, sp[11:] + sp[:11]))
        text = "\n".join(fmt.format(i=i, a=a[0], b=b[0]) for i, (a, b) in enumerate(use)).encode()
        got = _ingest(ctx, spec, text)
        _assert_oracle(got, _oracle(spec, text), spec)
        _assert_bits(got["x"], [a[1] for a, _ in use], "x against Python", [a[0] for a, _ in use])
        _assert_bits(got["y"], [b[1] for _, b in use], "y against Python", [b[0] for _, b in use])


@pytest.mark.parametrize("spec", [C.CSV_T, C.CSV, C.TSV, C.WKT, C.GEO], ids=["csv_t", "csv", "tsv", "wkt", "geojson"])
def test_known_answers_as_batches(ctx, spec):
    """The KNOWN table of test_ingest.py through the kernels: records with an answer mixed into one
    batch of ordinary records; a record the reference throws on alone in a batch, named by index."""
    sd = _specs(spec)[0]
    mine = [(rec, want, may) for s, rec, want, may in C.KNOWN if s == spec]
    good = [(rec, want) for rec, want, may in mine
            if want is not None and not (may and _abi.debug_ingest_record(sd, rec) is None)]
    lines = [C.ordinary_record(spec, i) for i in range(3000)]
    at = [10 + 61 * j for j in range(len(good))]
    for a, (rec, _) in zip(at, good):
        lines[a] = rec
    text = b"\n".join(lines)
    got = _ingest(ctx, spec, text)
    _assert_oracle(got, _oracle(spec, text), spec)
    _assert_bits(got["x"][at], [w[0] for _, w in good], "x against the known answers")
    _assert_bits(got["y"][at], [w[1] for _, w in good], "y against the known answers")
    if spec[4] >= 0:
        assert got["ts"][at].tolist() == [w[2] for _, w in good]
    for j, (rec, want, may) in enumerate(mine):
        if want is None or (may and _abi.debug_ingest_record(sd, rec) is None):
            bad_lines, bad_at = _lone_bad(ctx, spec, rec, j)
            if want is None:
                with pytest.raises(cref.IngestRejected) as e:
                    cref.ingest(_specs(spec)[1], b"\n".join(bad_lines))
                assert e.value.bad == bad_at


def _traj(ctx, text, spec_args, off=None):
    traj_d = _abi.make_traj_spec(utc_offset_min=off) if off is not None else None
    traj_o = cref.traj_spec(utc_offset_min=off) if off is not None else None
    got = ctx.ingest_trajectory(_abi.make_ingest_spec(*spec_args), _device_text(text), None, traj_d, with_ts=True)
    want = cref.ingest_traj(cref.ingest_spec(*spec_args), traj_o, text)
    assert len(got["x"]) == len(want["x"])
    _assert_bits(got["x"].cpu().numpy(), want["x"], "x against the oracle")
    _assert_bits(got["y"].cpu().numpy(), want["y"], "y against the oracle")
    ts = got["ts"].cpu().numpy()
    assert np.array_equal(ts, want["ts"])
    return ts


@pytest.mark.parametrize("off", [-720, 0, 330, 840])
def test_trajectory_lenient_dates(ctx, off):
    """GeoJSON 'timestamp' strings through parse_date_ymd_hms: years 1583-9999, every field at 00,
    01, 12, 13, 31, 59, 60 and 99 (the lenient calendar carries them), four zone offsets, and
    strings the reference's caught ParseException turns into 0."""
    dates = C.date_strings() + list(C.DATE_ZERO)
    text = b"\n".join(C.date_record(s, i) for i, s in enumerate(dates))
    ts = _traj(ctx, text, (cref.GEOJSON,), off)
    nz = len(C.DATE_ZERO)
    assert not ts[-nz:].any() and np.count_nonzero(ts[:-nz]) >= len(ts) - nz - 1
    py = [C.date_millis(s, off) for s in dates[:-nz]]
    known = np.array([p is not None for p in py])
    assert known.sum() > 0.9 * len(py)
    assert np.array_equal(ts[:-nz][known], np.array([p for p in py if p is not None], dtype=np.int64))
    # a raw control character inside a JSON string: the reference's Jackson parser throws
    lines = [C.date_record(s, i) for i, s in enumerate(dates[:200])]
    for j, s in enumerate(C.DATE_CONTROL):
        bad = list(lines)
        bad[(j * 37 + 11) % 200] = C.date_record(s, j)
        with pytest.raises(_abi.GeohipUnsupportedError) as d:
            ctx.ingest_trajectory(_abi.make_ingest_spec(cref.GEOJSON), _device_text(b"\n".join(bad)), None,
                                  _abi.make_traj_spec(utc_offset_min=off))
        assert d.value.bad == (j * 37 + 11) % 200, s


def test_trajectory_long_timestamps(ctx):
    """CSV timestamps through parse_long: +-(2^63 - 1), -2^63, 18 and 19 digits, -0, +5, leading
    zeros; 2^63 and beyond are rejected by index."""
    lines = [C.ordinary_record(C.CSV_T, i) for i in range(3000)]
    at = [5 + 131 * j for j in range(len(C.LONG_OK))]
    for a, t in zip(at, C.LONG_OK):
        lines[a] = f"v{a},{t},116.5,39.75".encode()
    ts = _traj(ctx, b"\n".join(lines), (cref.CSV, ",", 2, 3, 1, 0))
    assert ts[at].tolist() == [int(t) for t in C.LONG_OK]
    for j, t in enumerate(C.LONG_BAD):
        bad_at = (j * 389 + 3) % 3000
        bad = list(lines)
        bad[bad_at] = f"v,{t},116.5,39.75".encode()
        with pytest.raises(_abi.GeohipUnsupportedError) as d:
            ctx.ingest_trajectory(_abi.make_ingest_spec(cref.CSV, ",", 2, 3, 1, 0), _device_text(b"\n".join(bad)))
        assert d.value.bad == bad_at, t
        with pytest.raises(cref.IngestRejected) as e:
            cref.ingest_traj(cref.ingest_spec(cref.CSV, ",", 2, 3, 1, 0), None, b"\n".join(bad))
        assert e.value.bad == bad_at, t


# ---- 3. cells of extreme coordinates --------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["wkt", "csv"])
@pytest.mark.parametrize("grid", ["beijing", "unit"])
def test_cells_of_extreme_coordinates(ctx, grid, fmt):
    """java_cell as compiled for the device: (int) saturation for +-Infinity / +-1e308 / +-1e300,
    NaN -> 0, and the values up to three ulps either side of the grid edges and five cell edges."""
    mx, my, l, n = GRIDS[grid]
    xs, ys = C.cell_axis_values(mx, l, n), C.cell_axis_values(my, l, n)
    pairs = [(a, b) for a in xs for b in ys]
    if fmt == "wkt":
        spec, text = C.WKT, "\n".join(f"POINT ({a} {b})" for a, b in pairs).encode()
    else:
        spec, text = C.CSV_T, "\n".join(f"{i},{i},{a},{b}" for i, (a, b) in enumerate(pairs)).encode()
    got = _ingest(ctx, spec, text, grid=GRIDS[grid])
    want = _oracle(spec, text, grid=GRIDS[grid])
    _assert_oracle(got, want, spec, cell=True)
    _assert_bits(got["x"], _floats([a for a, _ in pairs]), "x against float()")
    _assert_bits(got["y"], _floats([b for _, b in pairs]), "y against float()")
    cells = set(want["cell"].tolist())
    assert 0xFFFFFFFF in cells and 0 in cells and len(cells) > 30  # outside, the NaN corner, many inside


# ---- 4. chunk geometry as it is today -------------------------------------------------------------

def _rounds(count):
    return -(-int(count) // THREADS)


@pytest.mark.parametrize("length,rounds", [(6, 8), (7, 7), (8, 6), (12, 4), (24, 2), (5, None)])
def test_hot_loop_rounds(ctx, length, rounds):
    """Fixed-length records: 6 bytes put exactly kFastStarts record starts in a chunk (8 rounds of
    the hot kernel's loop; chunk 0 owns byte 0 as well, so it is one past the edge and goes whole
    to ingest_general), 7 / 8 / 12 / 24 bytes give 7 / 6 / 4 / 2 rounds, 5 bytes overfill every chunk."""
    n = min(200_000, 4_000_000 // length)
    text = C.fixed_records(length, n)
    assert len(text) == n * length
    counts = C.chunk_record_counts(text)
    full = counts[1:-1]
    if rounds is None:
        assert (full > FAST_STARTS).all()
    else:
        assert (full <= FAST_STARTS).all() and {_rounds(c) for c in full} == {rounds}
    if length == 6:
        assert counts[0] == FAST_STARTS + 1 and (full == FAST_STARTS).all()
    spec = ("csv", ",", 0, 1, -1)
    got = _ingest(ctx, spec, text)
    _assert_oracle(got, _oracle(spec, text), spec)
    fx, fy = C.fixed_values(length, n)
    _assert_bits(got["x"], fx, "x against the generator")
    _assert_bits(got["y"], fy, "y against the generator")


def test_neighbouring_chunks_take_different_routes(ctx):
    """Stretches of 6-byte records (the hot kernel, 8 rounds) and of 5-byte records (overfull
    chunks, ingest_general) alternate, so the look-back chains chunks of both kinds."""
    parts, fx, fy, first = [], [], [], 0
    for k in range(18):
        length, n = (6, 10000) if k % 2 == 0 else (5, 12000)
        parts.append(C.fixed_records(length, n, first))
        a, b = C.fixed_values(length, n, first)
        fx.append(a)
        fy.append(b)
        first += n
    text = b"".join(parts)
    counts = C.chunk_record_counts(text)
    hot = counts[1:-1] <= FAST_STARTS
    assert hot.sum() >= 8 and (~hot).sum() >= 8 and np.count_nonzero(hot[1:] != hot[:-1]) >= 16
    spec = ("csv", ",", 0, 1, -1)
    got = _ingest(ctx, spec, text)
    _assert_oracle(got, _oracle(spec, text), spec)
    _assert_bits(got["x"], np.concatenate(fx), "x against the generator")
    _assert_bits(got["y"], np.concatenate(fy), "y against the generator")


@pytest.mark.parametrize("pad", [0, 700], ids=["short", "past_tail"])
def test_chunk_boundary_sweep(ctx, pad):
    """A tie-token record starting at every offset from chunk_end - 130 to chunk_end + 2 (133 chunk
    ends): records straddling a chunk end are parsed from the staged tail by the chunk that owns
    them; with a 700-character objID they run past chunk + tail (CHUNK + TAIL staged bytes), so
    fast_csv gives up at the staged end and LdsReader reads the rest from global memory."""
    text, rows, xt, yt = C.boundary_sweep(pad)
    assert 133 * CHUNK < len(text) < 4_000_000
    if pad:
        assert pad + 40 - 130 > TAIL  # even the earliest of them ends past chunk + tail
    got = _ingest(ctx, C.CSV_T, text)
    _assert_oracle(got, _oracle(C.CSV_T, text), C.CSV_T)
    _assert_bits(got["x"][rows], _floats(xt), "x against float()", xt)
    _assert_bits(got["y"][rows], _floats(yt), "y against float()", yt)


def test_batch_end_sweep(ctx):
    """Where the batch ends inside the staged window the staged end is the batch end: a tie-token
    record with 0 .. 130 bytes after it crosses swar_csv's 112-byte record span and, with no '\\n'
    after it, fast_csv's end-of-stage test."""
    n = 0
    for text, row, a, b in C.batch_end_sweep():
        got = _ingest(ctx, C.CSV_T, text)
        _assert_oracle(got, _oracle(C.CSV_T, text), C.CSV_T)
        _assert_bits(got["x"][row:row + 1], [float(a)], "x against float()", [a])
        _assert_bits(got["y"][row:row + 1], [float(b)], "y against float()", [b])
        n += 1
    assert n == 125
