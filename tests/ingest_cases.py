"""Case generators shared by the CPU and GPU tests of the ingest codec (a plain module).

tests/test_ingest.py runs these cases through the host-compiled record parser
(``_abi.debug_ingest_record``), tests/test_gpu_ingest_numeric.py runs the same cases through the
gfx950 kernels, so both draw from one place: the hand-derived known answers (``KNOWN``), the
decimal / halfway / hex fuzz generators, and the number corpus of plain ``-?digits(.digits)?``
tokens with the three record layouts that steer it through the kernels' three conversion sites.

Nothing here imports the product or the oracle: expected values of number tokens are Python
``float(token)`` / ``float.fromhex`` (correctly rounded, independent of the project).
"""
from __future__ import annotations

import functools
import random
from decimal import Decimal, localcontext

import numpy as np

NAN = float("nan")
INF = float("inf")

# Chunk geometry of the kernels, written once: spatialflink_amd/csrc/ingest.h:20-21
# (kIngestChunk = 512 * 48, kIngestTail) and ingest.hip:339 (kFastStarts); ingest.hip:193-194
# (kSwarRecordSpan, kSwarFieldSpan) and the 24-byte field window of swar_csv (ingest.hip:196).
CHUNK = 24576
TAIL = 512
FAST_STARTS = 4096
THREADS = 512
SWAR_RECORD_SPAN = 112
SWAR_FIELD_SPAN = 72
SWAR_WINDOW = 24

FMT_ID = {"csv": 0, "geojson": 1, "wkt": 2}

# ATC-style CSVTSVToTSpatial schema: [oid, ts, x, y] -> csvTsvSchemaAttr = [0, 1, 2, 3]
CSV_T = ("csv", ",", 2, 3, 1)
CSV = ("csv", ",", 2, 3, -1)
TSV = ("csv", "\t", 0, 1, -1)
WKT = ("wkt", ",", 0, 1, -1)
GEO = ("geojson", ",", 0, 1, -1)

# (spec, record, expected (x, y, ts) or None where the reference throws, device-may-reject)
# device-may-reject: valid Java input outside the device grammar (the batch call then returns
# GEOHIP_ERR_UNSUPPORTED and the caller hands the batch to the reference deserializer).
KNOWN = [
    (CSV_T, b"7,1611022449423,116.4148990000001,39.92037412345", (116.4148990000001, 39.92037412345, 1611022449423), False),
    (CSV_T, b'"7","1611022449423","116.5","39.75"', (116.5, 39.75, 1611022449423), False),
    (CSV_T, b"7 , 12 , 116.5 , 39.75", (116.5, 39.75, 12), False),
    (CSV_T, b"7,12,116.5", None, False),  # get(3): IndexOutOfBoundsException
    (CSV_T, b"7,12,116.5,abc", None, False),  # NumberFormatException
    (CSV_T, b"7,12,1e3,-2.5E-1", (1000.0, -0.25, 12), False),
    (CSV_T, b"7,12,+1.5d,2f", (1.5, 2.0, 12), False),  # Java type suffixes
    (CSV_T, b"7,12,NaN,-Infinity", (NAN, -INF, 12), False),
    (CSV_T, b"7,12,.5,5.", (0.5, 5.0, 12), False),
    (CSV_T, b"7,12,.,1", None, False),
    (CSV_T, b"7,12,1e,1", None, False),
    (CSV_T, b"7,12,nan,1", None, False),  # NaN is case-sensitive
    (CSV_T, b"7,12,1.5\x01,2", (1.5, 2.0, 12), False),  # Double.valueOf trims every char <= ' '
    (CSV_T, b"7,+12,1,2", (1.0, 2.0, 12), False),
    (CSV_T, b"7,12.0,1,2", None, False),  # Long.valueOf
    (CSV_T, b"7, 12\x01,1,2", None, False),  # Long.valueOf does not trim
    (CSV_T, b"7,9223372036854775808,1,2", None, False),  # Long overflow
    (CSV_T, b"7,-9223372036854775808,1,2", (1.0, 2.0, -9223372036854775808), False),
    (CSV_T, b"7,9223372036854775807,1,2", (1.0, 2.0, 9223372036854775807), False),
    (CSV_T, b"7,12,0x1.8p1,2", (3.0, 2.0, 12), False),  # hex significand
    (CSV_T, b"7,12,-0X.8P-1d,0x1p-1074", (-0.25, 5e-324, 12), False),
    (CSV_T, b"7,12,0x1p-1075,0x1.0000000000001p-1075", (0.0, 5e-324, 12), False),  # tie to even / just above
    (CSV_T, b"7,12,0x1.fffffffffffff8p1023,0x1p99999999999", (INF, INF, 12), False),  # rounds past MAX / int range
    (CSV_T, b"7,12,0x0.0p5,-0x1p-99999999999", (0.0, -0.0, 12), False),
    (CSV_T, b"7,12,0x1.00000000000008p0,0x1.00000000000018p0", (1.0, 1.0000000000000004, 12), False),  # ties
    (CSV_T, b"7,12,0x123456789abcdef0123p-70,2", (float.fromhex("0x123456789abcdef0123p-70"), 2.0, 12), False),
    (CSV_T, b"7,12,0xp1,2", None, False),
    (CSV_T, b"7,12,0x1.8p,2", None, False),
    (CSV_T, b"7,12,0x1.8,2", None, False),  # hex needs a binary exponent
    (CSV_T, b"7,12,1.5,2,extra", (1.5, 2.0, 12), False),
    (CSV_T, b",12,1,2", (1.0, 2.0, 12), False),  # leading "" field
    (CSV_T, b"7,12,0.1,0.30000000000000004", (0.1, 0.30000000000000004, 12), False),
    (CSV_T, b"7,12,9007199254740993,2", (9007199254740992.0, 2.0, 12), False),  # tie -> even
    (CSV_T, b"7,12,1.000000000000000000000001,2", (1.0, 2.0, 12), False),  # 25 digits, decided by truncation
    (CSV_T, b"7,12,2.2250738585072011e-308,4.9e-324", (2.225073858507201e-308, 5e-324, 12), False),
    (CSV_T, b"7,12,1e400,1e-400", (INF, 0.0, 12), False),
    (CSV_T, b"7,12,-0.0,0", (-0.0, 0.0, 12), False),
    (CSV_T, b"7,12,1e1000000,2", (INF, 2.0, 12), False),  # 7-digit exponent
    (CSV_T, b"7,12,1e-99999999999999,0e99999999999", (0.0, 0.0, 12), False),
    (CSV_T, b"7,12,-0.001e1000000002,2", (-INF, 2.0, 12), False),
    (CSV_T, b'7,12,1"5,2', (15.0, 2.0, 12), False),  # quotes deleted inside a token
    (CSV_T, b'7,1"2,-"1".5"e1,2', (-15.0, 2.0, 12), False),
    (CSV_T, b"7,12,1 5,2", None, False),
    (CSV, b"a,b,116.5,39.75", (116.5, 39.75, 0), False),
    (CSV, b"a,b,116.5,", None, False),  # trailing "" removed -> get(3) throws
    (CSV, b"a,b,116.5,\t", None, False),
    (TSV, b"116.5\t39.75", (116.5, 39.75, 0), False),
    (TSV, b"116.5 \t 39.75", (116.5, 39.75, 0), False),
    (TSV, b"116.5 39.75", None, False),  # no tab: one field
    (TSV, b" 116.5\t39.75 ", (116.5, 39.75, 0), False),
    (TSV, b'116.5"\t"39.75', (116.5, 39.75, 0), False),
    (WKT, b"POINT (116.5 39.75)", (116.5, 39.75, 0), False),
    (WKT, b"POINT(116.5 39.75)", (116.5, 39.75, 0), False),
    (WKT, b"id,POINT ( 116.5   39.75 ) trailing", (116.5, 39.75, 0), False),
    (WKT, b"POINT (116.5,39.75)", None, False),
    (WKT, b"POINT EMPTY", None, False),
    (WKT, b"MULTIPOINT ((1 2))", None, False),
    (WKT, b"POINT (1 2 3)", (1.0, 2.0, 0), False),
    (WKT, b"POINT (nan NaN 0x1p4)", (NAN, NAN, 0), False),  # WKTReader: NaN ignoring case
    (WKT, b"POINT (1 2 3 4)", None, False),
    (WKT, b"POINT (1 2 x)", None, False),
    (WKT, b"POINT (1.5d -2e1)", (1.5, -20.0, 0), False),
    (WKT, b"point (1 2)", None, False),
    (WKT, b"POINTZ (1 2)", None, False),
    (GEO, b'{"geometry":{"coordinates":[116.44412,39.93984],"type":"Point"},"properties":{"oID":"2560",'
          b'"timestamp":"2008-02-02 20:12:32"},"type":"Feature"}', (116.44412, 39.93984, 0), False),
    (GEO, b'{"type":"Point","coordinates":[1,2]}', (1.0, 2.0, 0), False),
    (GEO, b'{"type":"Point","coordinates":[ -0 , 2.5e-1 ]}', (0.0, 0.25, 0), False),  # IntNode 0
    (GEO, b'{"type":"Point","coordinates":[-0.0,1]}', (-0.0, 1.0, 0), False),
    (GEO, b'{"type":"Point","coordinates":[01,2]}', None, False),
    (GEO, b'{"type":"Point","coordinates":[+1,2]}', None, False),
    (GEO, b'{"type":"Point","coordinates":[1.,2]}', None, False),
    (GEO, b'{"type":"LineString","coordinates":[[1,2],[3,4]]}', (1.0, 2.0, 0), False),
    (GEO, b'{"type":"Point","coordinates":[1e400,2]}', None, False),
    (GEO, b'{"type":"Point","coordinates":[9223372036854775807,-9223372036854775808]}',
     (9.223372036854776e18, -9.223372036854776e18, 0), False),  # LongNode
    (GEO, b'{"type":"Point","coordinates":[9223372036854775808,1]}', None, False),  # BigIntegerNode
]


# ---- fuzz generators of tests/test_ingest.py -------------------------------------------------

def _rand_decimal(rng: random.Random) -> str:
    nint = rng.choice([0, 1, 1, 2, 3, 5, 10, 17, 20])
    nfrac = rng.choice([0, 1, 2, 5, 10, 13, 16, 17, 19, 22])
    if nint + nfrac == 0:
        nint = 1
    ip = "".join(rng.choice("0123456789") for _ in range(nint))
    fp = "".join(rng.choice("0123456789") for _ in range(nfrac))
    s = ip + ("." + fp if nfrac or rng.random() < 0.1 else "")
    if rng.random() < 0.4:
        s += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.choice([0, 1, 5, 22, 23, 100, 290, 300, 307, 308,
                                                                                  309, 320, 324, 330, 340, 350]))
    if rng.random() < 0.3:
        s = rng.choice("+-") + s
    return s


def decimal_fuzz_pairs(n=20000, seed=20260116):
    """The (a, b) token pairs of test_decimal_conversion_fuzz, in its order."""
    rng = random.Random(seed)
    return [(_rand_decimal(rng), _rand_decimal(rng)) for _ in range(n)]


def sig_digits(tok: str) -> int:
    """Significant digits of a decimal token as the parser counts them (from the first non-zero)."""
    return len(tok.lstrip("+-").split("e")[0].split("E")[0].replace(".", "").lstrip("0"))


def halfway_values():
    rng = np.random.default_rng(7)
    return rng.uniform(-1e3, 1e3, 300).tolist() + [1.0, 0.1, 116.41, 39.92, 5e-324, 1e300, 2.0 ** -1022]


def halfway_tokens(vals=None):
    """(token, digits) for points at (and 1e-35 relative around) the midpoint of adjacent doubles,
    written with digits + 1 = 17, 18, 21 and 41 significant digits."""
    vals = halfway_values() if vals is None else vals
    out = []
    with localcontext() as c:
        c.prec = 80
        for v in vals:
            mid = (Decimal(v) + Decimal(float(np.nextafter(v, np.inf)))) / 2
            for t in (mid, mid * (1 + Decimal(10) ** -35), mid * (1 - Decimal(10) ** -35)):
                for digits in (16, 17, 20, 40):
                    out.append((format(t, f".{digits}e"), digits))
    return out


def hex_or_long_exponent_token(rng: random.Random):
    """(token, expected double): a hex significand (Double.parseDouble's parseHexString grammar)
    or a decimal token with a long exponent."""
    if rng.random() < 0.7:
        ih = "".join(rng.choice("0123456789abcdefABCDEF") for _ in range(rng.choice([0, 1, 2, 7, 14, 16, 20])))
        fh = "".join(rng.choice("0123456789abcdef") for _ in range(rng.choice([0, 1, 3, 13, 15, 20])))
        if not ih and not fh:
            ih = "1"
        body = ih + ("." + fh if fh or rng.random() < 0.2 else "")
        ex = rng.choice([0, 1, -1, 52, -1022, -1074, -1075, -1080, 1023, 1024, -1100, 900, -990,
                         rng.randint(-1200, 1200)])
        t = rng.choice(["", "-", "+"]) + rng.choice(["0x", "0X"]) + body + rng.choice("pP") + str(ex)
        t += rng.choice(["", "", "d", "F"])
        try:
            want = float.fromhex(t.rstrip("dF"))
        except OverflowError:
            want = -INF if t.startswith("-") else INF
    else:
        m = rng.choice(["1", "0", "0.0", "7.25", "123456789", "0.000001"])
        e = rng.choice([1000000, 99999999, 123456789012, -1000000, -99999999999])
        t = rng.choice(["", "-"]) + m + "e" + str(e)
        want = float(t)
    return t, want


def hex_fuzz_pairs(n=20000, seed=424242):
    """The ((token, want), (token, want)) pairs of test_hex_and_long_exponent_fuzz, in its order."""
    rng = random.Random(seed)
    return [(hex_or_long_exponent_token(rng), hex_or_long_exponent_token(rng)) for _ in range(n)]


# ---- the number corpus: plain '-'? digits ('.' digits)? tokens, <= 19 significant digits ------

def all_digits(tok: str) -> int:
    """Digits of a plain token counting leading zeros (swar_csv's budget, ingest.hip:301)."""
    return sum(c.isdigit() for c in tok)


def swar_takes(tok: str) -> bool:
    """swar_csv's own acceptance of a number field: at most 19 digits counting leading zeros
    (ingest.hip:301) and its terminator inside the 24-byte window (ingest.hip:289, 296)."""
    return all_digits(tok) <= 19 and len(tok) < SWAR_WINDOW


def _digits(rng, n, first_nonzero=True):
    s = "".join(rng.choice("0123456789") for _ in range(n))
    if first_nonzero and n and s[0] == "0":
        s = rng.choice("123456789") + s[1:]
    return s


def _plain(v: float) -> str:
    """Shortest repr of v written without an exponent."""
    s = format(Decimal(repr(v)), "f")
    return s


@functools.lru_cache(maxsize=None)
def number_corpus(seed=20261020):
    """[(class, token)]: classes 'a' digit splits, 'b' ties, 'c' neighbours of powers of two and
    ten, 'd' small magnitudes (long fractions), 'e' signs.  Every token has at most 19 significant
    digits, so the host-compiled parser must decide every one of them."""
    rng = random.Random(seed)
    out = []
    # (a) every (ni, nf) split of the 19-digit budget
    for ni in range(1, 20):
        for nf in range(0, 20 - ni):
            def tok(first_nonzero=True):
                ip = _digits(rng, ni, first_nonzero and ni > 1)
                return ip + ("." + _digits(rng, nf, False) if nf else "")
            for _ in range(80):
                out.append(("a", tok()))
            out.append(("a", "9" * ni + ("." + "9" * nf if nf else "")))
            if nf:
                out.append(("a", _digits(rng, ni, ni > 1) + "." + "0" * nf))
            for k in (1, 2, 3):  # leading zeros inside swar_csv's 19-digit limit
                if k + ni + nf <= 19:
                    out.append(("a", "0" * k + tok()))
                    out.append(("a", "0" * k + tok()))
            for k in (20 - ni - nf, 25, 40):  # more leading zeros: only fast_csv accepts those
                out.append(("a", "0" * k + tok()))
                out.append(("a", "0" * k + tok()))
    # (b) ties: odd multiples of half an ulp above 2^53 .. 2^63, with .0 / .00 / .000 (q = -1..-3)
    for e in range(53, 64):
        half = 1 << (e - 53)
        kmax = min(1 << 52, (10 ** 19 - (1 << e)) // (2 * half) - 1)
        ks = list(range(6)) + [rng.randrange(kmax) for _ in range(30)] + [kmax - 1 - j for j in range(4)]
        for k in ks:
            t = (1 << e) + (2 * k + 1) * half
            for d in (0, -1, 1):
                s = str(t + d)
                assert len(s) <= 19
                out.append(("b", s))
                for z in (1, 2, 3):
                    if len(s) + z <= 19:
                        out.append(("b", s + "." + "0" * z))
    for _ in range(300):  # x.5 between the integers x and x + 1 of [2^52, 2^53), and 1e-3 either side
        x = rng.randrange(1 << 52, 1 << 53)
        out += [("b", f"{x}.5"), ("b", f"{x}.500"), ("b", f"{x}.499"), ("b", f"{x}.501")]
    # (c) neighbours of powers of two and ten that fit in 19 digits without an exponent
    for v in [2.0 ** e for e in range(-40, 64)] + [10.0 ** e for e in range(-22, 19)]:
        for u in (v, float(np.nextafter(v, np.inf)), float(np.nextafter(v, -np.inf))):
            s = _plain(u)
            if sig_digits(s) <= 19 and u < 1e19:
                out.append(("c", s))
    # (d) small magnitudes: "0." + z zeros + digits, down through the subnormals to underflow
    for z in range(0, 346):
        for _ in range(5):
            out.append(("d", "0." + "0" * z + _digits(rng, rng.randint(1, 19))))
    for z, ds in ((307, ["22250738585072014", "22250738585072013", "22250738585072015", "2225073858507201383",
                         "2225073858507201384", "2225073858507201400", "2225073858507201399", "2225073858507200889",
                         "2225073858507200890", "22250738585072009", "22250738585072011"]),
                  (323, ["2470328229206232720", "2470328229206232721", "2470328229206232719", "24703282292062327",
                         "24703282292062328", "5", "4", "3", "2", "25", "24", "49", "74", "75", "7410984687618698162",
                         "7410984687618698163", "9881312916824930883", "1"]),
                  (324, ["2470328229206232720", "9999999999999999999", "1"]),
                  (341, ["1", "9"]), (342, ["1"]), (345, ["9999999999999999999"])):
        for s in ds:
            out.append(("d", "0." + "0" * z + s))
    # (e) signs
    sample = rng.sample(out, 3000)
    out += [("e", t) for t in ("-0", "-0.0", "-0.000", "0", "0.0", "-0." + "0" * 30)]
    out += [("e", "-" + t) for _, t in sample]
    for _, t in out:
        assert sig_digits(t) <= 19, t
    return tuple(out)


def _ts_of(i: int) -> int:
    """Timestamps of at most 18 digits (both fast paths take them, ingest.hip:153, 301)."""
    return (1611022449423 + i, -(i + 1), 10 ** 17 + i, 0)[i % 4]


FILLER = "f,1611022449423,116.5,39.75"
MARKERS = ('"q","1611022449423","116.25",39.5', "q , 1611022449423 , 116.25 , 39.5")


def layout(kind: str, swap: bool, seed=20261020):
    """The number corpus as one 'id,ts,x,y' CSV batch laid out for one conversion site.

    kind 'swar': short fields; 'fast': a 30-character objID in field 0; 'general': short fields
    plus a quoted / blank-padded marker record often enough that every chunk holds one.
    Every corpus token is paired with a short partner token, so a record is shorter than the
    staged tail; swap puts the partner first, so every token runs in both number columns.
    Returns (text, rows, xtok, ytok): record index and the two tokens of every corpus record."""
    corpus = [t for _, t in number_corpus(seed)]
    short = [t for t in corpus if swar_takes(t)]
    if kind == "swar":
        corpus = short
    lines, rows, xt, yt = [], [], [], []
    since_marker, nm = None, 0
    for i, t in enumerate(corpus):
        if kind == "general" and (since_marker is None or since_marker >= 8000):
            lines.append(MARKERS[nm % 2])
            nm += 1
            since_marker = 0
        a, b = t, short[(i * 7919) % len(short)]
        if swap:
            a, b = b, a
        oid = f"v{i:029d}" if kind == "fast" else str(i % 1000)
        rec = f"{oid},{_ts_of(i)},{a},{b}"
        rows.append(len(lines))
        lines.append(rec)
        xt.append(a)
        yt.append(b)
        if since_marker is not None:
            since_marker += len(rec) + 1
    # ordinary records past the last corpus record: 112 staged bytes or more follow each of those
    lines += [FILLER] * 6
    if kind == "general":
        lines.append(MARKERS[0])
    text = ("\n".join(lines) + "\n").encode()
    return text, np.array(rows), xt, yt


def record_starts(text: bytes) -> np.ndarray:
    b = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(b[:-1] == 10)  # a '\n' at the last byte ends the last record
    return np.concatenate([[0], nl + 1]) if len(text) else np.zeros(0, dtype=np.int64)


def owner_chunk(starts: np.ndarray) -> np.ndarray:
    """The chunk that owns each record: the one holding the '\n' before it (ingest.h:14-16)."""
    return np.where(starts == 0, 0, (starts - 1) // CHUNK)


def check_layout(kind: str, text: bytes, rows: np.ndarray) -> None:
    """The path a layout forces, restated from the kernels' acceptance rules and asserted on the
    text itself (nothing measures which path ran)."""
    starts = record_starts(text)
    own = owner_chunk(starts)
    staged_end = np.minimum((own + 1) * CHUNK + TAIL, len(text))
    ends = np.concatenate([starts[1:] - 1, [len(text) - 1]])  # each record's '\n'
    recs = text.split(b"\n")[:-1]
    assert len(recs) == len(starts)
    if kind == "general":
        marked = np.array([r.startswith((b'"', b"q ")) for r in recs])
        # every chunk that owns a record owns an undecided one: ingest.hip:462-467 lists the chunk,
        # ingest.hip:490-499 re-parses all of its records with parse_record
        assert set(own.tolist()) == set(own[marked].tolist())
        return
    for r in rows.tolist():
        rec, s = recs[r], int(starts[r])
        f = rec.split(b",")
        assert len(f) == 4 and all(32 < c < 127 and c != 34 for c in rec)
        # fast_csv: the whole record, its '\n' included, inside the staged bytes (ingest.hip:151, 168)
        assert ends[r] < staged_end[r]
        assert all(sig_digits(t.decode()) <= 19 for t in f[2:]) and all_digits(f[1].decode()) <= 18
        if kind == "swar":
            # ingest.hip:273 (record span), :280 (field starts), :289 / :296 / :316 (terminator in the
            # 24-byte window), :301 (19 digits counting leading zeros)
            assert s + SWAR_RECORD_SPAN <= staged_end[r]
            assert all(len(t) < SWAR_WINDOW for t in f)
            assert all(all_digits(t.decode()) <= 19 for t in f[2:])
            assert len(rec) - len(f[3]) <= SWAR_FIELD_SPAN
        else:
            # ingest.hip:313-316: no stop byte in field 0's 24-byte window -> kSwarNo -> fast_csv
            assert len(f[0]) >= SWAR_WINDOW


# ---- the general grammar: batches for ingest_general ------------------------------------------

def large_value_tokens():
    """(token, expected): DBL_MAX in 309 digits, half an ulp above it, huge exponents."""
    dbl_max = int(float.fromhex("0x1.fffffffffffffp1023"))
    half_ulp = 1 << (1023 - 53)
    toks = [str(dbl_max), str(dbl_max + half_ulp), str(dbl_max + half_ulp - 1), str(dbl_max - 1), str(dbl_max) + ".0",
            "1e308", "1e309", "1.7976931348623157e308", "1.7976931348623159e308", "1" + "0" * 400, "1" + "0" * 308,
            "1e1000000", "1e-99999999999", "-1e1000000", "0e1000000", "-0e-99999999999", "123456789e99999999",
            "0." + "0" * 400 + "1", "0." + "0" * 400 + "1e400", "1" + "0" * 400 + "e-400"]
    out = []
    for t in toks:
        try:
            want = float(t)
        except OverflowError:  # Python raises only for int literals, which these are not
            want = INF
        out.append((t, want))
    return out


def large_value_batch(n=5000, seed=31):
    """[((tok, want), (tok, want))]: every large token once in each column, among decimal fuzz."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        a, b = _rand_decimal(rng), _rand_decimal(rng)
        out.append(((a, float(a)), (b, float(b))))
    for j, tw in enumerate(large_value_tokens()):
        out[100 + 97 * j] = (tw, out[100 + 97 * j][1])
        out[150 + 97 * j] = (out[150 + 97 * j][0], tw)
    return out


def special_tokens():
    """(token, expected): NaN, Infinity, Java type suffixes, a leading '+', '.5' and '5.'."""
    out = [("NaN", NAN), ("+NaN", NAN), ("-NaN", NAN), ("Infinity", INF), ("+Infinity", INF), ("-Infinity", -INF)]
    for body in ("1.5", "2", ".5", "5.", "1e3", "0.1", "116.4148990000001", "9007199254740993", "4.9e-324"):
        for sign in ("", "+", "-"):
            for suf in ("", "d", "D", "f", "F"):
                out.append((sign + body + suf, float(sign + body)))
    return out


# ---- TrajectoryStream: lenient dates (parse_date_ymd_hms) and Long timestamps (parse_long) -----

DATE_PAIRS = ("00", "01", "12", "13", "31", "59", "60", "99")
DATE_YEARS = (1583, 1600, 1900, 1970, 2000, 2038, 9999)
DATE_ZERO = ("", "abc", " ", "x2008-02-02 20:12:32", "T12", "/", "   ")  # ParseException -> 0
# a raw control character inside a JSON string: Jackson throws before the map function runs
DATE_CONTROL = ("  \t", "\t", "a\tb", "2008-02-02 20:12:32\r", "\x01", "2008-02-02\x1f20:12:32")


def date_strings(seed=5):
    """'yyyy-MM-dd HH:mm:ss' strings: every listed digit pair in every field of every listed year
    (the other fields random pairs), everyday dates, and random mixes."""
    rng = random.Random(seed)
    out = []
    for y in DATE_YEARS:
        out.append(f"{y:04d}-01-01 00:00:00")
        out.append(f"{y:04d}-12-31 23:59:59")
        out.append(f"{y:04d}-02-29 12:00:00")
        for pos in range(5):
            for p in DATE_PAIRS:
                f = [rng.choice(DATE_PAIRS) for _ in range(5)]
                f[pos] = p
                out.append(f"{y:04d}-{f[0]}-{f[1]} {f[2]}:{f[3]}:{f[4]}")
    for _ in range(1500):
        f = [rng.choice(DATE_PAIRS) if rng.random() < 0.5 else f"{rng.randrange(100):02d}" for _ in range(5)]
        out.append(f"{rng.choice(DATE_YEARS) if rng.random() < 0.5 else rng.randrange(1583, 10000):04d}"
                   f"-{f[0]}-{f[1]} {f[2]}:{f[3]}:{f[4]}")
    return out


def date_millis(s: str, off_min: int):
    """Epoch milliseconds of a lenient 'yyyy-MM-dd HH:mm:ss' by Python's own calendar (None where
    the carried year leaves datetime's range)."""
    import datetime
    y, mo, d = int(s[0:4]), int(s[5:7]), int(s[8:10])
    h, mi, sec = int(s[11:13]), int(s[14:16]), int(s[17:19])
    y2, m2 = y + (mo - 1) // 12, (mo - 1) % 12 + 1  # month 00: December of the year before
    if not 1 <= y2 <= 9999:
        return None
    days = datetime.date(y2, m2, 1).toordinal() - datetime.date(1970, 1, 1).toordinal() + d - 1
    return (((days * 24 + h) * 60 + mi) * 60 + sec - off_min * 60) * 1000


def date_record(s: str, i: int) -> bytes:
    return ('{"type":"Feature","geometry":{"type":"Point","coordinates":[116.5,39.9]},"properties":{"oID":"%d",'
            '"timestamp":"%s"}}' % (i, s)).encode()


LONG_OK = [str(2 ** 63 - 1), str(-(2 ** 63 - 1)), str(-2 ** 63), "9" * 18, "-" + "9" * 18, "1" + "0" * 18,
           "-1" + "0" * 18, "1" + "0" * 17, "9223372036854775806", "-0", "+0", "+5", "0005", "0" * 30 + "7",
           "-" + "0" * 25 + "9223372036854775808", "+9223372036854775807", "123456789012345678", "1234567890123456789"]
LONG_BAD = [str(2 ** 63), str(-2 ** 63 - 1), "9" * 19, "9" * 20, "+" + str(2 ** 63), "18446744073709551616", "-", "+"]


def ordinary_record(spec, i: int) -> bytes:
    """An everyday record of the spec's format (Beijing coordinates)."""
    x, y = 115.5 + (i * 7919 % 21000) / 1e4, 39.6 + (i * 104729 % 15000) / 1e4
    if spec[0] == "wkt":
        return f"POINT ({x!r} {y!r})".encode()
    if spec[0] == "geojson":
        return ('{"type":"Point","coordinates":[%r,%r]}' % (x, y)).encode()
    if spec[1] == "\t":
        return f"{x!r}\t{y!r}".encode()
    return f"{i},{1611022449423 + i},{x!r},{y!r}".encode()


# ---- chunk geometry: fixed-length records, the chunk-boundary sweep ---------------------------

def fixed_records(length: int, n: int, first=0) -> bytes:
    """n records 'digits,digits\\n' of exactly `length` bytes each (fx = 0, fy = 1, no timestamp)."""
    wb = (length - 2) // 2
    wa = length - 2 - wb
    return b"".join(b"%0*d,%0*d\n" % (wa, (i * 7919) % 10 ** wa, wb, (i * 104729) % 10 ** wb)
                    for i in range(first, first + n))


def fixed_values(length: int, n: int, first=0):
    wb = (length - 2) // 2
    wa = length - 2 - wb
    i = np.arange(first, first + n, dtype=np.int64)
    return ((i * 7919) % 10 ** wa).astype(np.float64), ((i * 104729) % 10 ** wb).astype(np.float64)


def chunk_record_counts(text: bytes) -> np.ndarray:
    return np.bincount(owner_chunk(record_starts(text)), minlength=(len(text) + CHUNK - 1) // CHUNK)


def tie_tokens():
    return [t for c, t in number_corpus() if c == "b"]


def _fill_to(lines, pos, target):
    """Ordinary records from byte pos up to exactly byte target (target - pos >= 28)."""
    gap = target - pos
    assert gap >= len(FILLER) + 1
    while gap >= 2 * (len(FILLER) + 1):
        lines.append(FILLER)
        gap -= len(FILLER) + 1
    lines.append("f" * (gap - len(FILLER) - 1) + FILLER)  # one record of exactly gap bytes with its '\n'
    return target


def boundary_sweep(pad: int):
    """One batch in which a hard-number record (corpus (b) tokens) starts at every offset from
    chunk_end - 130 to chunk_end + 2, one chunk end per offset; pad > 0 gives those records an
    objID of pad characters, so the ones near a chunk end run past chunk + tail.
    Returns (text, rows, xtok, ytok)."""
    ties = tie_tokens()
    lines, rows, xt, yt = [], [], [], []
    pos = 0
    for j, off in enumerate(range(-130, 3)):
        target = (j + 1) * CHUNK + off
        pos = _fill_to(lines, pos, target)
        a, b = ties[(j * 31) % len(ties)], ties[(j * 17 + 5) % len(ties)]
        rec = f"{'p' * pad if pad else j % 10},{_ts_of(j)},{a},{b}"
        rows.append(len(lines))
        lines.append(rec)
        xt.append(a)
        yt.append(b)
        pos += len(rec) + 1
    lines += [FILLER] * 6
    text = ("\n".join(lines) + "\n").encode()
    starts = record_starts(text)
    assert [int(starts[r]) - (j + 1) * CHUNK for j, r in enumerate(rows)] == list(range(-130, 3))
    return text, np.array(rows), xt, yt


def batch_end_sweep():
    """Small batches whose hard-number record has t = 0, 1, 8 .. 130 bytes after it before the
    batch ends: the staged end is the batch end here, so the record crosses kSwarRecordSpan
    (ingest.hip:273) and, with no '\\n' after it (t = 0), fast_csv's p >= lim (ingest.hip:151).
    Yields (text, row, xtok, ytok)."""
    ties = tie_tokens()
    for n, t in enumerate([0, 1] + list(range(8, 131))):
        a, b = ties[(n * 13 + 1) % len(ties)], ties[(n * 29 + 7) % len(ties)]
        lines = [FILLER] * 20 + [f"{n % 10},{_ts_of(n)},{a},{b}"]
        text = "\n".join(lines)
        if t >= 1:
            text += "\n"
        if t >= 8:
            text += "f" * (t - 1 - 6) + ",1,2,3"  # a last record of t - 1 bytes, no '\n' after it
        yield text.encode(), 20, a, b


# ---- cells of extreme coordinates -------------------------------------------------------------

def cell_axis_values(mn: float, l: float, n: int):
    """Tokens for one axis: NaN, +-Infinity, +-1e308, +-1e300, and the values up to three ulps either
    side of both grid edges and of five interior cell edges."""
    toks = ["NaN", "Infinity", "-Infinity", "1e308", "-1e308", "1e300", "-1e300"]
    for k in (0, n, 1, 17, 50, 83, 99):
        e = mn + k * l
        lo = hi = e
        vals = [e]
        for _ in range(3):
            lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))
            vals += [lo, hi]
        toks += [repr(v) for v in vals]
    return toks
