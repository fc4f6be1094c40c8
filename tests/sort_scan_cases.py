"""The case table of tests/test_gpu_sort_scan_edges.py: seeded inputs for gsr_sort_pairs_u64_u32 and gsr_inclusive_scan_u32 at
the structural edges of csrc/radix_sort.hip and csrc/scan.hip, and their references in numpy. No GPU, no torch:
tests/test_sort_scan_cases_cpu.py proves that every case has the property it is named for."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

# The kernels' constants, mirrored here and nowhere else in the tests.
SORT_TILE = 8192            # radix_sort.hip kSortTile: keys per workgroup and ticket (kThreads 512 x kItems 16)
WAVE_SPAN = 1024            # radix_sort.hip kWaveSpan: keys of a tile that one wave ranks (kWave 64 x kItems 16)
XCD_GROUP = 64              # radix_sort.hip 8 * kXcdRun: tiles of one full group of take_tile's remapping
DIGIT_BITS = 8              # radix_sort.hip launch_sort_pairs: bits per pass; the last pass takes what is left (1..8)
MIN_RADIX_BITS = 4          # radix_sort.hip radix_bits_for: the narrowest pass kernel (widths 1..3 run on it with nbins < RADIX)
TICKET_WORDS = 8            # radix_sort.hip take_tile: one ticket per residue class blockIdx % 8, or the first one alone
SCAN_TILE = 4096            # scan.hip kScanTile: elements per workgroup of tile_reduce / tile_scan
SCAN_THREADS = 1024         # scan.hip partial_scan_kernel's launch bounds: thread t owns tiles [t per, (t + 1) per)
SCAN_MAX_PER = 16           # scan.hip kMaxPer: tiles per thread kept in registers; beyond it the other body of the kernel runs

U64_MAX = (1 << 64) - 1


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def mask(width: int) -> int:
    return (1 << width) - 1


def documented_window(begin_bit: int, end_bit: int) -> tuple[int, int]:
    """(begin, width) of the bits that take part, as include/gsrast_amd.h documents the clamping of gsr_sort_pairs_u64_u32."""
    end_bit = min(end_bit, 64)
    begin_bit = max(begin_bit, 0)
    if end_bit <= begin_bit:
        end_bit = begin_bit + 1
    return begin_bit, end_bit - begin_bit


def pass_widths(width: int) -> list[int]:
    """Digit widths of the passes of a window, lowest digit first."""
    return [min(DIGIT_BITS, width - s) for s in range(0, width, DIGIT_BITS)]


def field_of(keys: np.ndarray, begin: int, width: int) -> np.ndarray:
    return (keys >> np.uint64(begin)) & np.uint64(mask(width))


def sort_reference(keys: np.ndarray, values: np.ndarray, begin: int, width: int) -> tuple[np.ndarray, np.ndarray]:
    order = np.argsort(field_of(keys, begin, width), kind="stable")
    return keys[order], values[order]


def scan_reference(x: np.ndarray) -> np.ndarray:
    return (np.cumsum(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- sort cases ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SortCase:
    name: str
    dist: str
    n: int
    begin_bit: int              # as passed to the entry point
    end_bit: int
    claims: tuple = ()          # what tests/test_sort_scan_cases_cpu.py proves of the inputs: see CLAIMS

    @property
    def window(self) -> tuple[int, int]:
        return documented_window(self.begin_bit, self.end_bit)

    @property
    def tiles(self) -> int:
        return ceil_div(self.n, SORT_TILE)

    def __str__(self) -> str:
        return self.name


CLAIMS = ("all_bits_live",      # every one of the 64 key bits is set in some key and clear in some key
          "all_equal",          # one key value
          "two_values",         # exactly two key values, whose fields differ
          "hot_tile",           # in every pass some tile of the INPUT holds one digit only
          "ascending",          # the fields never decrease, and do increase
          "descending",
          "low_byte_cycle",     # the field is i % 256
          "top_in_partial")     # the last tile is partial and holds real keys with the top digit of every pass


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


def _random_u64(rng, n: int) -> np.ndarray:
    return rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)


def _with_field(background: np.ndarray, field: np.ndarray, begin: int, width: int) -> np.ndarray:
    """`background` with its bits [begin, begin + width) replaced by `field`: the bits outside the window stay live."""
    window = np.uint64(mask(width) << begin)
    return (background & ~window) | ((field.astype(np.uint64) << np.uint64(begin)) & window)


def _values(rng, n: int) -> np.ndarray:
    """Random u32 with repeats, among them 0 and 0xFFFFFFFF (both present from n = 2 on)."""
    v = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    pool = np.array([0, 0xFFFFFFFF, 0x80000000, 7], np.uint32)
    pick = rng.random(n) < 0.25
    v[pick] = rng.choice(pool, int(pick.sum()))
    if n >= 2:
        v[(n - 1) // 2] = 0
        v[-1] = 0xFFFFFFFF
    return v


HOT_TILE = 1                    # the tile of the hot-digit inputs that holds the hot key only
LAST_TOP_KEYS = 100             # "top_last": how many keys at the end have every window bit set


def _ramp(n: int, width: int) -> np.ndarray:
    """n fields that never fall, from 0 up to (nearly) the window's largest value; nothing overflows 64 bits (n < 2^24)."""
    top, i = mask(width), np.arange(n, dtype=np.uint64)
    return i * np.uint64(top) // np.uint64(n - 1) if width <= 40 else i * np.uint64(top // (n - 1))


@functools.lru_cache(maxsize=4)
def _sort_inputs(dist: str, n: int, begin: int, width: int) -> tuple[np.ndarray, np.ndarray]:
    # (the random keys do not depend on the window: every window case sorts the same keys)
    rng = np.random.default_rng(_seed(dist, n) if dist == "random" else _seed(dist, n, begin, width))
    values = _values(rng, n)
    if dist == "random":
        keys = _random_u64(rng, n)
    elif dist == "all_equal":
        keys = np.full(n, 0xC3A5_0F96_D2E1_78B4, np.uint64)
    elif dist == "alternating":
        a = 0x9E37_79B9_7F4A_7C15
        keys = np.where(np.arange(n) % 2 == 0, np.uint64(a), np.uint64(a ^ U64_MAX))
    elif dist == "hot_digit":
        keys = np.full(n, 0x5DA7_13C8_6EB2_F049, np.uint64)
        outside = np.nonzero(np.arange(n) // SORT_TILE != HOT_TILE)[0]
        cold = rng.choice(outside, max(n // 100, 1), replace=False)
        keys[cold] = _random_u64(rng, len(cold))
    elif dist == "ascending":
        keys = _with_field(_random_u64(rng, n), _ramp(n, width), begin, width)
    elif dist == "descending":
        keys = _with_field(_random_u64(rng, n), _ramp(n, width)[::-1], begin, width)
    elif dist == "low_byte_cycle":
        keys = (np.arange(n, dtype=np.uint64) % np.uint64(256)) << np.uint64(begin)
    elif dist == "top_all":
        keys = _with_field(_random_u64(rng, n), np.full(n, mask(width), np.uint64), begin, width)
    elif dist == "top_last":
        keys = _random_u64(rng, n)
        keys[-LAST_TOP_KEYS:] |= np.uint64(mask(width) << begin)
    else:
        raise ValueError(dist)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys.setflags(write=False)
    values.setflags(write=False)
    return keys, values


def sort_inputs(case: SortCase) -> tuple[np.ndarray, np.ndarray]:
    """(keys u64[n], values u32[n]) of a case: read-only, the same arrays whenever it is asked for."""
    begin, width = case.window
    if case.dist == "random":
        begin, width = 0, 64
    return _sort_inputs(case.dist, case.n, begin, width)


# sizes, window [0, 64), full-random keys: (n, tiles). Around one wave's span, one tile, and every tile count at which
# take_tile's `full` changes; 127 and 129 tiles complete the list of counts around the second group.
SORT_SIZES = ((1, 1), (2, 1), (63, 1), (64, 1), (65, 1),
              (WAVE_SPAN - 1, 1), (WAVE_SPAN, 1), (WAVE_SPAN + 1, 1),
              (SORT_TILE - 1, 1), (SORT_TILE, 1), (SORT_TILE + 1, 2),
              (2 * SORT_TILE - 1, 2), (2 * SORT_TILE + 1, 3),
              (63 * SORT_TILE, 63), (63 * SORT_TILE + 1, 64), (64 * SORT_TILE - 1, 64), (64 * SORT_TILE, 64),
              (64 * SORT_TILE + 1, 65), (65 * SORT_TILE + 7, 66), (127 * SORT_TILE, 127), (127 * SORT_TILE + 1, 128),
              (128 * SORT_TILE, 128), (129 * SORT_TILE, 129), (129 * SORT_TILE + 1, 130))
ALL_BITS_LIVE_FROM = 63         # (two keys cannot have every bit both set and clear... 63 random keys do, but for 2^-56)
SIZE_CASES = tuple(SortCase(f"n{n}", "random", n, 0, 64, ("all_bits_live",) if n >= ALL_BITS_LIVE_FROM else ())
                   for n, _ in SORT_SIZES)

# bit windows: every width 1..17 at begins that are and are not byte-aligned, and ending at bit 64
WINDOW_N = 3 * SORT_TILE + 5
WINDOW_WIDTHS = tuple(range(1, 18))
WINDOW_BEGINS = (0, 3, 8, 29, 32, 37, 47)


def _window_cases():
    out = []
    for width in WINDOW_WIDTHS:
        for begin in sorted(set(WINDOW_BEGINS) | {64 - width}):
            out.append(SortCase(f"w{width}_b{begin}", "random", WINDOW_N, begin, min(begin + width, 64), ("all_bits_live",)))
    return tuple(out)


WINDOW_CASES = _window_cases()

# the clamping at the top of launch_sort_pairs: (case, the window include/gsrast_amd.h documents for it)
CLAMP_CASES = ((SortCase("end70", "random", WINDOW_N, 0, 70, ("all_bits_live",)), (0, 64)),
               (SortCase("end70_b52", "random", WINDOW_N, 52, 70, ("all_bits_live",)), (52, 12)),
               (SortCase("begin-5", "random", WINDOW_N, -5, 13, ("all_bits_live",)), (0, 13)),
               (SortCase("end_eq_begin", "random", WINDOW_N, 20, 20, ("all_bits_live",)), (20, 1)),
               (SortCase("end_below_begin", "random", WINDOW_N, 40, 8, ("all_bits_live",)), (40, 1)))

DIST_SIZES = (2 * SORT_TILE + 3, 65 * SORT_TILE + 1)
DIST_WINDOWS = ((0, 64), (32, 45))
DIST_CLAIMS = {"all_equal": ("all_equal",), "alternating": ("two_values",), "hot_digit": ("hot_tile",),
               "ascending": ("ascending",), "descending": ("descending",), "low_byte_cycle": ("low_byte_cycle",),
               "top_all": ("top_in_partial",), "top_last": ("top_in_partial",)}
DIST_CASES = tuple(SortCase(f"{dist}_n{n}_b{b}_e{e}", dist, n, b, e, claims)
                   for dist, claims in DIST_CLAIMS.items() for n in DIST_SIZES for b, e in DIST_WINDOWS)

# rerun with one ticket (GSR_SORT_SINGLE_TICKET=1): the sizes from 63 tiles upward, the hot digit, all keys equal
SINGLE_TICKET_CASES = tuple(c for c in SIZE_CASES if c.n >= 63 * SORT_TILE) + \
    tuple(c for c in DIST_CASES if c.dist in ("hot_digit", "all_equal"))

SORT_CASES = SIZE_CASES + WINDOW_CASES + tuple(c for c, _ in CLAMP_CASES) + DIST_CASES


def ticket_words_offset(n: int) -> int:
    """Where in `temp` the sort keeps its tickets (radix_sort.hip launch_sort_pairs: behind the spare keys and the spare
    values, each rounded up to 128 bytes; carve_sweep_scratch puts the tickets first)."""
    return ceil_div(8 * n, 128) * 128 + ceil_div(4 * n, 128) * 128


def tickets_after(tiles: int, single: bool) -> list[int]:
    """The ticket words after a pass of `tiles` workgroups (take_tile): every workgroup has drawn once — from the first
    ticket alone, or from the ticket of its residue class."""
    return [tiles] + [0] * (TICKET_WORDS - 1) if single else [len(range(r, tiles, TICKET_WORDS)) for r in range(TICKET_WORDS)]


# ---- scan cases ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScanCase:
    name: str
    pattern: str
    n: int
    claims: tuple = ()          # "wraps": the un-wrapped total exceeds 2^32; "per_gt_max": the kernel's re-reading body runs

    @property
    def tiles(self) -> int:
        return ceil_div(self.n, SCAN_TILE)

    @property
    def per(self) -> int:
        return ceil_div(self.tiles, SCAN_THREADS)

    def __str__(self) -> str:
        return self.name


@functools.lru_cache(maxsize=1)
def _scan_input(pattern: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(_seed("scan", pattern, n))
    if pattern == "random":
        x = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    elif pattern == "below_4096":
        x = rng.integers(0, 1 << 12, size=n, dtype=np.uint32)
    elif pattern == "all_ones_bits":
        x = np.full(n, 0xFFFFFFFF, np.uint32)
    elif pattern == "zeros":
        x = np.zeros(n, np.uint32)
    elif pattern == "one_first":
        x = np.zeros(n, np.uint32)
        x[0] = 1
    elif pattern == "one_last":
        x = np.zeros(n, np.uint32)
        x[-1] = 1
    else:
        raise ValueError(pattern)
    x.setflags(write=False)
    return x


def scan_input(case: ScanCase) -> np.ndarray:
    return _scan_input(case.pattern, case.n)


@functools.lru_cache(maxsize=1)
def scan_expected(case: ScanCase) -> np.ndarray:
    """scan_reference of the case's input, computed once for the tests that share it."""
    ref = scan_reference(scan_input(case))
    ref.setflags(write=False)
    return ref


# (n, tiles, per): around the lane's vector, the wave, the chunk and the tile, and around 1024 tiles (per 1 -> 2)
SCAN_SIZES = ((1, 1, 1), (2, 1, 1), (3, 1, 1), (4, 1, 1), (5, 1, 1), (255, 1, 1), (256, 1, 1), (257, 1, 1),
              (1023, 1, 1), (1024, 1, 1), (1025, 1, 1), (SCAN_TILE - 1, 1, 1), (SCAN_TILE, 1, 1), (SCAN_TILE + 1, 2, 1),
              (2 * SCAN_TILE - 1, 2, 1), (2 * SCAN_TILE + 1, 3, 1),
              (1024 * SCAN_TILE - 1, 1024, 1), (1024 * SCAN_TILE, 1024, 1), (1024 * SCAN_TILE + 1, 1025, 2),
              (1025 * SCAN_TILE + 3, 1026, 2))
SCAN_WRAPS_FROM = 5             # (five random u32 exceed 2^32 in all but one draw of 120; the seeds here do)
SCAN_VALUE_CASES = tuple(ScanCase(f"n{n}", "random", n, ("wraps",) if n >= SCAN_WRAPS_FROM else ()) for n, _, _ in SCAN_SIZES)
SCAN_PATTERN_SIZES = (SCAN_TILE + 1, 1025 * SCAN_TILE + 3)
SCAN_PATTERN_CASES = tuple(ScanCase(f"{p}_n{n}", p, n, ("wraps",) if p == "all_ones_bits" else ())
                           for n in SCAN_PATTERN_SIZES for p in ("all_ones_bits", "zeros", "one_first", "one_last"))
# The body of partial_scan_kernel for per > kMaxPer: (n, tiles, per, the first thread that owns no tile, tiles of the last owner)
SCAN_BIG = ((SCAN_MAX_PER * SCAN_THREADS * SCAN_TILE + 1, 16385, 17, 964, 14),
            (17 * SCAN_THREADS * SCAN_TILE + 5, 17409, 18, 968, 3))
SCAN_BIG_CASES = tuple(ScanCase(f"n{n}", "below_4096", n, ("wraps", "per_gt_max")) for n, *_ in SCAN_BIG)
SCAN_CASES = SCAN_VALUE_CASES + SCAN_PATTERN_CASES + SCAN_BIG_CASES
