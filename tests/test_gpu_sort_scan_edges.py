"""GPU: gsr_sort_pairs_u64_u32 (csrc/radix_sort.hip) and gsr_inclusive_scan_u32 (csrc/scan.hip) through the C entry points,
bit for bit against numpy, at the structural edges tests/sort_scan_cases.py lists (tests/test_sort_scan_cases_cpu.py proves each
case has its property). Every array of a call is carved from one buffer of sentinel bytes with a gap on both sides; `temp` is
exactly gsr_*_temp_bytes(n) long and full of 0xFF bytes — what a previous call's status words, tickets and counts look like at
their worst — so a call that writes outside its arrays, or reads a word of `temp` it did not clear, fails."""
import numpy as np
import pytest

import sort_scan_cases as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5                 # every byte of the buffer that belongs to no array
GAP = 512                       # sentinel bytes on both sides of every array (arrays start on 128-byte boundaries)
POISON = 0x5A                   # outputs before the call
DIRTY = 0xFF                    # temp before the call


class _Arena:
    """One device buffer of SENTINEL bytes; every named array is a slice of exactly its size with at least GAP sentinel bytes
    on both sides. An array is given as a numpy array (copied in) or as (bytes, fill byte)."""

    def __init__(self, **arrays):
        import torch
        self.slices, at = {}, GAP
        for name, a in arrays.items():
            nbytes = a.nbytes if isinstance(a, np.ndarray) else a[0]
            self.slices[name] = slice(at, at + nbytes)
            at = (at + nbytes + GAP + 127) // 128 * 128
        self.dev = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % 128 == 0
        for name, a in arrays.items():
            if isinstance(a, np.ndarray):
                self.dev[self.slices[name]] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
            else:
                self.dev[self.slices[name]] = a[1]

    def ptr(self, name):
        return self.dev.data_ptr() + self.slices[name].start

    def read(self, name, dtype):
        return self.dev[self.slices[name]].cpu().numpy().view(dtype)

    def gaps_intact(self):
        """Every byte outside the arrays still holds the sentinel (compared on the device: only the verdict comes back)."""
        import torch
        torch.cuda.synchronize()
        at, ok = 0, True
        for q in list(self.slices.values()) + [slice(self.dev.numel(), None)]:
            ok = ok and bool((self.dev[at:q.start] == SENTINEL).all())
            at = q.stop
        return ok


def _sort(keys, values, begin_bit, end_bit, want_tickets=False):
    """One call on fresh buffers with every guard; returns (keys_out, values_out[, the ticket words left in temp])."""
    import torch
    from gsrast_amd import _capi
    n = len(keys)
    temp_bytes = int(_capi.lib().gsr_sort_temp_bytes(n))
    assert temp_bytes >= 12 * n
    arena = _Arena(keys_in=keys, keys_out=(8 * n, POISON), values_in=values, temp=(temp_bytes, DIRTY), values_out=(4 * n, POISON))
    _capi.call("gsr_sort_pairs_u64_u32", arena.ptr("keys_in"), arena.ptr("keys_out"), arena.ptr("values_in"), arena.ptr("values_out"),
               n, begin_bit, end_bit, arena.ptr("temp"), _capi.stream(arena.dev.device), device=arena.dev.device)
    torch.cuda.synchronize()
    assert arena.gaps_intact(), "the sort wrote outside its outputs and gsr_sort_temp_bytes(n) of temp"
    assert np.array_equal(arena.read("keys_in", np.uint64), keys), "keys_in is not preserved"
    assert np.array_equal(arena.read("values_in", np.uint32), values), "values_in is not preserved"
    out = (arena.read("keys_out", np.uint64), arena.read("values_out", np.uint32))
    if want_tickets:
        at = S.ticket_words_offset(n)
        out += (arena.read("temp", np.uint8)[at:at + 4 * S.TICKET_WORDS].view(np.uint32).tolist(),)
    return out


def _first_difference(got, want):
    bad = np.nonzero(got != want)[0]
    return None if len(bad) == 0 else (int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), len(bad))


def _check_sort(case, window=None):
    keys, values = S.sort_inputs(case)
    begin, width = window or case.window
    got_keys, got_values = _sort(keys, values, case.begin_bit, case.end_bit)
    want_keys, want_values = S.sort_reference(keys, values, begin, width)
    # (index, got, expected, how many differ)
    assert _first_difference(got_keys, want_keys) is None, "keys"
    assert _first_difference(got_values, want_values) is None, "values"
    return got_keys, got_values


@pytest.mark.parametrize("case", S.SIZE_CASES, ids=str)
def test_sort_sizes(case):
    """Full-random u64 keys on bits [0, 64): eight live passes, around the wave span, the tile and take_tile's groups of 64."""
    _check_sort(case)


@pytest.mark.parametrize("case", S.WINDOW_CASES, ids=str)
def test_sort_bit_windows(case):
    """Every last-pass width 1..8 behind zero, one and two full passes, at begins that are not byte-aligned; the bits outside
    the window are live and must neither move equal fields nor change."""
    _check_sort(case)


@pytest.mark.parametrize("case,window", S.CLAMP_CASES, ids=[str(c) for c, _ in S.CLAMP_CASES])
def test_sort_clamps_its_window_as_documented(case, window):
    """end_bit > 64, begin_bit < 0, end_bit <= begin_bit: the window include/gsrast_amd.h documents."""
    _check_sort(case, window)


@pytest.mark.parametrize("case", S.DIST_CASES, ids=str)
def test_sort_distributions(case):
    got_keys, got_values = _check_sort(case)
    if case.dist == "all_equal":
        assert np.array_equal(got_values, S.sort_inputs(case)[1])           # (nothing moves)


@pytest.mark.parametrize("case", S.SINGLE_TICKET_CASES, ids=str)
def test_sort_single_ticket(case, library_env):
    """take_tile's single ticket (devices below 64 compute units), switched on here by GSR_SORT_SINGLE_TICKET=1: the same
    result as the reference and, bit for bit, as with the tickets per XCD residue class. The ticket words the last pass
    leaves in temp tell that each call took the branch it was asked for."""
    keys, values = S.sort_inputs(case)
    begin, width = case.window
    want_keys, want_values = S.sort_reference(keys, values, begin, width)
    got = {}
    for single in (0, 1):
        library_env(GSR_SORT_SINGLE_TICKET=str(single))
        got_keys, got_values, tickets = _sort(keys, values, case.begin_bit, case.end_bit, want_tickets=True)
        assert tickets == S.tickets_after(case.tiles, bool(single)), (single, tickets)
        assert _first_difference(got_keys, want_keys) is None, ("keys", single)
        assert _first_difference(got_values, want_values) is None, ("values", single)
        got[single] = (got_keys, got_values)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def _scan(x, in_place):
    import torch
    from gsrast_amd import _capi
    n = len(x)
    temp_bytes = int(_capi.lib().gsr_scan_temp_bytes(n))
    assert temp_bytes >= 4 * S.ceil_div(n, S.SCAN_TILE)
    arrays = dict(x=x, temp=(temp_bytes, DIRTY))
    if not in_place:
        arrays["out"] = (4 * n, POISON)
    arena = _Arena(**arrays)
    _capi.call("gsr_inclusive_scan_u32", arena.ptr("x"), arena.ptr("x" if in_place else "out"), n, arena.ptr("temp"),
               _capi.stream(arena.dev.device), device=arena.dev.device)
    torch.cuda.synchronize()
    assert arena.gaps_intact(), "the scan wrote outside its output and gsr_scan_temp_bytes(n) of temp"
    if not in_place:
        assert np.array_equal(arena.read("x", np.uint32), x), "the input is not preserved"
    got = arena.read("x" if in_place else "out", np.uint32)
    del arena
    return got


@pytest.mark.parametrize("in_place", (False, True), ids=("separate", "in_place"))
@pytest.mark.parametrize("case", S.SCAN_VALUE_CASES + S.SCAN_PATTERN_CASES, ids=str)
def test_scan_values(case, in_place):
    """Full-range u32 (the sum wraps at every other element) around the vector, wave, chunk and tile sizes and around 1024
    tiles, where a thread of partial_scan_kernel starts to own two; all ones, all zero and a lone 1 at either end."""
    x = S.scan_input(case)
    assert _first_difference(_scan(x, in_place), S.scan_expected(case)) is None


@pytest.mark.parametrize("in_place", (False, True), ids=("separate", "in_place"))
@pytest.mark.parametrize("case", S.SCAN_BIG_CASES, ids=str)
def test_scan_beyond_sixteen_tiles_per_thread(case, in_place):
    """More than 16 tiles per thread of partial_scan_kernel (67 M elements and more, 268 MB each way): its re-reading body,
    with threads that own no tile and a ragged last owner."""
    import torch
    x = S.scan_input(case)
    got = _scan(x, in_place)
    torch.cuda.empty_cache()                    # (the buffers of this case are gone before the next one allocates)
    assert _first_difference(got, S.scan_expected(case)) is None
