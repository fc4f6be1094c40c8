"""CPU: every case of tests/sort_scan_cases.py has the property it is named for, so that no case of
tests/test_gpu_sort_scan_edges.py can pass vacuously; and the references order equal fields as a stable sort does."""
import numpy as np
import pytest

import sort_scan_cases as S


def _digits(keys, begin, width):
    """Per pass of the window, lowest first: (digit width, the keys' digits)."""
    out, shift = [], begin
    for w in S.pass_widths(width):
        out.append((w, S.field_of(keys, shift, w)))
        shift += w
    return out


def test_sort_sizes_have_the_tile_counts_they_are_listed_with():
    assert len(S.SIZE_CASES) == len(S.SORT_SIZES)
    for case, (n, tiles) in zip(S.SIZE_CASES, S.SORT_SIZES):
        assert case.n == n and case.tiles == tiles == S.ceil_div(n, 8192), case.name
        assert case.window == (0, 64)
    # every count at which take_tile's number of remapped positions changes, and the counts beside them
    assert {1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130} <= {t for _, t in S.SORT_SIZES}
    full = {t // S.XCD_GROUP * S.XCD_GROUP for _, t in S.SORT_SIZES}
    assert full == {0, 64, 128}
    # ... with an empty, a one-tile and a longer incomplete group behind the full ones
    assert {t % S.XCD_GROUP for _, t in S.SORT_SIZES if t >= S.XCD_GROUP} >= {0, 1, 2, 63}
    # the sizes the issue names
    named = {1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16385, 63 * 8192, 63 * 8192 + 1, 64 * 8192 - 1,
             64 * 8192, 64 * 8192 + 1, 65 * 8192 + 7, 127 * 8192 + 1, 128 * 8192, 129 * 8192 + 1}
    assert named <= {n for n, _ in S.SORT_SIZES}
    assert S.ceil_div(S.WINDOW_N, 8192) == 4 and S.WINDOW_N == 3 * 8192 + 5
    assert S.DIST_SIZES == (2 * 8192 + 3, 65 * 8192 + 1)
    assert [S.ceil_div(n, 8192) for n in S.DIST_SIZES] == [3, 66]


def test_window_cases_reach_every_last_pass_width_after_zero_one_and_two_full_passes():
    reached, begins = set(), {}
    for case in S.WINDOW_CASES:
        begin, width = case.window
        assert (begin, width) == (case.begin_bit, case.end_bit - case.begin_bit) and begin + width <= 64, case.name
        widths = S.pass_widths(width)
        assert all(w == S.DIGIT_BITS for w in widths[:-1]) and sum(widths) == width
        reached.add((len(widths) - 1, widths[-1]))
        begins.setdefault(width, set()).add(begin)
    assert {(full, last) for full in (0, 1) for last in range(1, 9)} | {(2, 1)} <= reached
    assert len(S.WINDOW_CASES) == len({c.name for c in S.WINDOW_CASES})
    for width in range(1, 18):
        assert begins[width] == {0, 3, 8, 29, 32, 37, 47, 64 - width}, width
    # the widths below the narrowest kernel (nbins < RADIX) are among them
    assert {1, 2, 3} <= {S.pass_widths(c.window[1])[-1] for c in S.WINDOW_CASES} and S.MIN_RADIX_BITS == 4


def test_clamp_cases_name_the_documented_window():
    by_name = {c.name: (c, w) for c, w in S.CLAMP_CASES}
    assert by_name["end70"][0].end_bit == 70 and by_name["end70"][1] == (0, 64)
    assert by_name["begin-5"][0].begin_bit == -5 and by_name["begin-5"][1] == (0, 13)
    assert by_name["end_eq_begin"][1] == (20, 1) and by_name["end_below_begin"][1] == (40, 1)
    for case, window in S.CLAMP_CASES:
        assert case.window == window, case.name
        assert (case.begin_bit, case.end_bit) != (window[0], window[0] + window[1]), case.name      # (something IS clamped)


def test_values_are_random_with_repeats_zero_and_all_ones():
    for case in (S.SIZE_CASES[1], S.SIZE_CASES[4], S.WINDOW_CASES[0], S.DIST_CASES[0]):
        _, values = S.sort_inputs(case)
        assert values.dtype == np.uint32 and len(values) == case.n
        assert (values == 0).any() and (values == 0xFFFFFFFF).any(), case.name
        if case.n >= 64:
            assert len(np.unique(values)) < case.n and not np.array_equal(values, np.arange(case.n)), case.name


@pytest.mark.parametrize("case", S.SORT_CASES, ids=str)
def test_sort_case_has_its_property_and_a_stable_reference(case):
    keys, values = S.sort_inputs(case)
    begin, width = case.window
    assert keys.dtype == np.uint64 and keys.shape == values.shape == (case.n,)
    assert set(case.claims) <= set(S.CLAIMS)
    field = S.field_of(keys, begin, width)
    tiles, last = case.tiles, keys[(case.tiles - 1) * S.SORT_TILE:]
    for claim in case.claims:
        if claim == "all_bits_live":
            assert int(np.bitwise_or.reduce(keys)) == S.U64_MAX and int(np.bitwise_and.reduce(keys)) == 0
            assert ((keys >> np.uint64(63)) == 1).mean() > 0.25                      # (bit 63 in about half of them)
        elif claim == "all_equal":
            assert len(np.unique(keys)) == 1
        elif claim == "two_values":
            assert len(np.unique(keys)) == 2 and len(np.unique(field)) == 2 and (keys[::2] == keys[0]).all()
        elif claim == "hot_tile":
            assert tiles >= 2 and (keys != keys[S.HOT_TILE * S.SORT_TILE]).sum() == max(case.n // 100, 1)
            for w, d in _digits(keys, begin, width):
                full_tiles = d[:case.n // S.SORT_TILE * S.SORT_TILE].reshape(-1, S.SORT_TILE)
                hottest = max(int(np.bincount(t.astype(np.int64), minlength=1 << w).max()) for t in full_tiles)
                assert hottest == S.SORT_TILE, (w, hottest)
        elif claim == "ascending":
            assert (field[1:] >= field[:-1]).all() and field[-1] > field[0]
            assert len(np.unique(field)) > min(case.n, 1 << width) // 2
        elif claim == "descending":
            assert (field[1:] <= field[:-1]).all() and field[-1] < field[0]
        elif claim == "low_byte_cycle":
            assert np.array_equal(field, np.arange(case.n, dtype=np.uint64) % np.uint64(256))
            assert np.array_equal(keys, field << np.uint64(begin))
        elif claim == "top_in_partial":
            assert 0 < len(last) < S.SORT_TILE and case.n % S.SORT_TILE != 0
            for w, d in _digits(last, begin, width):
                # (the padding of the last tile is ranked in digit RADIX - 1 of the pass's kernel)
                assert w >= S.MIN_RADIX_BITS and (d == S.mask(w)).any(), w
            top = field == np.uint64(S.mask(width))
            assert top.all() if case.dist == "top_all" else (top[-S.LAST_TOP_KEYS:].all() and top.mean() < 0.01)
    # the bits outside a narrower window are live: they must ride along, and must not decide anything
    if width < 64 and case.dist in ("random", "ascending", "descending", "top_all", "top_last", "hot_digit", "alternating"):
        assert len(np.unique(keys & ~np.uint64(S.mask(width) << begin))) > 1
    # the reference: fields in order, equal fields in input order, and exactly the inputs permuted
    ref_keys, order = S.sort_reference(keys, np.arange(case.n, dtype=np.uint32), begin, width)
    sorted_field = S.field_of(ref_keys, begin, width)
    assert np.array_equal(ref_keys, keys[order])
    assert np.array_equal(np.sort(order), np.arange(case.n))
    rising = sorted_field[1:] > sorted_field[:-1]
    equal = sorted_field[1:] == sorted_field[:-1]
    assert (rising | equal).all() and (order[1:][equal] > order[:-1][equal]).all()
    if width < 64 and case.n > (1 << width):
        assert equal.any()                                                          # (there ARE ties to keep in order)
    _, ref_values = S.sort_reference(keys, values, begin, width)
    assert np.array_equal(ref_values, values[order])


def test_single_ticket_cases_are_the_named_ones():
    sizes = {c.n for c in S.SINGLE_TICKET_CASES if c.dist == "random"}
    assert sizes == {n for n, _ in S.SORT_SIZES if n >= 63 * 8192} and min(sizes) == 63 * 8192
    assert {c.dist for c in S.SINGLE_TICKET_CASES} == {"random", "hot_digit", "all_equal"}
    assert all(c in S.SIZE_CASES + S.DIST_CASES for c in S.SINGLE_TICKET_CASES)
    # what the ticket words hold after a pass, either way
    assert S.tickets_after(65, True) == [65, 0, 0, 0, 0, 0, 0, 0]
    assert S.tickets_after(65, False) == [9, 8, 8, 8, 8, 8, 8, 8] and S.tickets_after(3, False) == [1, 1, 1, 0, 0, 0, 0, 0]
    assert S.ticket_words_offset(3) == 128 + 128 and S.ticket_words_offset(8192) == 65536 + 32768


def test_scan_sizes_have_the_tiles_and_owners_they_are_listed_with():
    assert len(S.SCAN_VALUE_CASES) == len(S.SCAN_SIZES)
    for case, (n, tiles, per) in zip(S.SCAN_VALUE_CASES, S.SCAN_SIZES):
        assert case.n == n and case.tiles == tiles == S.ceil_div(n, 4096) and case.per == per == S.ceil_div(tiles, 1024), case.name
    named = {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 1024 * 4096 - 1, 1024 * 4096,
             1024 * 4096 + 1, 1025 * 4096 + 3}
    assert named == {n for n, _, _ in S.SCAN_SIZES}
    assert S.SCAN_PATTERN_SIZES == (4097, 1025 * 4096 + 3)
    assert {c.pattern for c in S.SCAN_PATTERN_CASES} == {"all_ones_bits", "zeros", "one_first", "one_last"}
    assert len(S.SCAN_PATTERN_CASES) == 8
    assert [n for n, *_ in S.SCAN_BIG] == [16384 * 4096 + 1, 17 * 1024 * 4096 + 5]
    for case, (n, tiles, per, first_idle, last_owns) in zip(S.SCAN_BIG_CASES, S.SCAN_BIG):
        assert case.n == n and case.tiles == tiles and case.per == per > S.SCAN_MAX_PER
        # partial_scan_kernel: t0 = min(t per, tiles), t1 = min(t0 + per, tiles)
        owned = [min(t * per + per, tiles) - min(t * per, tiles) for t in range(S.SCAN_THREADS)]
        assert sum(owned) == tiles and owned.index(0) == first_idle and owned[first_idle - 1] == last_owns
        assert all(o == 0 for o in owned[first_idle:]) and all(o == per for o in owned[:first_idle - 1])
    assert S.SCAN_BIG[0][4] < 17 and S.SCAN_BIG[1][4] < 18                          # (a ragged last owner in both)
    # the largest size that still takes the register body is one element below the first big case
    assert S.ceil_div(S.ceil_div(S.SCAN_BIG[0][0] - 1, 4096), 1024) == S.SCAN_MAX_PER


@pytest.mark.parametrize("case", S.SCAN_CASES, ids=str)
def test_scan_case_has_its_property(case):
    x = S.scan_input(case)
    assert x.dtype == np.uint32 and x.shape == (case.n,)
    total = int(x.sum(dtype=np.uint64))
    if "wraps" in case.claims:
        assert total > 1 << 32, total
    if case.pattern == "random" and case.n >= 256:
        assert x.max() > 0xF0000000 and total > case.n << 30                        # (full range: it wraps every other element)
    if case.pattern == "below_4096":
        assert x.max() == 4095 and total >> 32 > 16                                 # (many wraps, each inside a run of a million elements)
        assert "per_gt_max" in case.claims and case.per > S.SCAN_MAX_PER
    if case.pattern in ("one_first", "one_last"):
        assert total == 1 and x[0 if case.pattern == "one_first" else -1] == 1
    if case.n <= 2 * S.SCAN_TILE + 1:
        ref = S.scan_reference(x)
        assert ref.dtype == np.uint32 and int(ref[-1]) == total & 0xFFFFFFFF
        assert all(int(ref[i]) == sum(int(v) for v in x[:i + 1]) & 0xFFFFFFFF for i in range(0, case.n, max(case.n // 7, 1)))
