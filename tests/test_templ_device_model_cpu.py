"""
What tests/test_gpu_templ_device.py relies on, shown without a GPU:

  * tests/templ_device_model.py - the area resize as its definition in fractions, the integer downscale in literal loops, the
    views as index arithmetic - equals the host helpers (MTM.augment.resize_area / downscale / expand, mtm_oracle.downscale_area)
    byte for byte on every base and record of the table;
  * constructed contents against expectations written out by hand: ties of both roundings, saturation, zero, 0 / 1 and 0 / 255
    masks;
  * the 16 records (k, lr, ud) are the 8 views of the dihedral group, the right ones;
  * mtm_oracle's direct sums are Python-integer triple loops - what comparing whole maps bit for bit rests on;
  * the table covers what it is there for (a table edit cannot silently drop an edge), and its hand-written families and
    rm_nt values are what the restated placement rule gives.
"""
import numpy as np
import pytest

import mtm_oracle as O
import templ_device_model as M
from test_exact_kernels_cpu import _triple_loop


@pytest.fixture(scope="module")
def A():
    from MTM import augment
    return augment


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", M.NAMES)
def test_model_equals_host_helpers(A, name):
    cell = M.BY_NAME[name]
    bases = M.cell_bases(cell)
    spec = [("", r) for r in cell["recs"]]
    host = A.expand([("b",) + tuple(a for a in base if a is not None) for base in bases], spec)
    mine = M.expand(bases, cell["recs"])
    assert len(host) == len(mine) == len(bases) * len(cell["recs"])
    for i, (hu, mu) in enumerate(zip(host, mine)):
        assert _eq(hu[1], mu[0]), (name, i, "pixels")
        assert hu[1].shape[:2] == M.unit_shape(cell["bases"][i // len(cell["recs"])], cell["recs"][i % len(cell["recs"])])
        if mu[1] is not None:
            assert _eq(hu[2], mu[1]), (name, i, "mask")
    # the two resizes on their own, and the oracle's statement of the integer rule
    for px, mask in bases:
        for r in {r[3:] for r in cell["recs"]}:
            for a in (px, mask):
                if a is None:
                    continue
                if r[0] > 0:
                    assert _eq(M.area_resize_exact(a, r[0], r[1]), A.resize_area(a, r[0], r[1]))
                elif r[2] > 1:
                    want = M.downscale_int_exact(a, r[2])
                    assert _eq(want, A.downscale(a, r[2])) and _eq(want, O.downscale_area(a, r[2]))


def test_area_resize_is_the_literal_definition():
    """The shapes the issue names, upscaling included, on random, saturated and 0 / 255 contents - against a second, slower
    statement: every output pixel integrates a piecewise-constant function, sampled on the common grid of rows H x cols W."""
    rng = np.random.default_rng(5)
    for (H, W), (rows, cols) in (((7, 5), (3, 4)), ((7, 5), (14, 10)), ((7, 5), (1, 1)), ((5, 9), (9, 5)), ((3, 3), (7, 2))):
        for a in (rng.integers(0, 256, (H, W)).astype(np.uint8), np.full((H, W), 255, np.uint8),
                  (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)):
            fine = np.repeat(np.repeat(a.astype(np.int64), rows, axis=0), cols, axis=1)          # (H rows) x (W cols) samples
            got = M.area_resize_exact(a, rows, cols)
            for i in range(rows):
                for j in range(cols):
                    blk = fine[i * H:(i + 1) * H, j * W:(j + 1) * W]
                    s = blk.reshape(H * W, -1).sum(axis=0)
                    want = [(2 * int(v) + H * W) // (2 * H * W) for v in s]
                    assert np.atleast_1d(got[i, j]).tolist() == want, ((H, W), (rows, cols), i, j)


# ---- constructed contents ---------------------------------------------------------------------------------------------------
def test_ties_of_the_integer_rule():
    """Factor 2 rounds a mean of k + 1/2 up; factors 3, 5 and 7 cannot meet a tie: s / f^2 is never k + 1/2 for odd f, and no
    rounding of the float32 product makes one (every sum 0 .. 255 f^2 enumerated) - the rule is then plain rounding of the
    exact mean, which the sums next to a tie pin from both sides."""
    ties2, _ = M.tie_sums(2)
    assert ties2 == list(range(2, 1021, 4)) and all(M.downscale_sum_rule(s, 2) == (s + 2) // 4 == s // 4 + 1 for s in ties2)
    for f in (3, 5, 7):
        ties, near = M.tie_sums(f)
        assert ties == [], (f, ties[:5])
        assert len(near) == 2 * 255 and near[:2] == [(f * f - 1) // 2, (f * f + 1) // 2]
        for s in range(255 * f * f + 1):
            assert M.downscale_sum_rule(s, f) == (2 * s + f * f) // (2 * f * f), (f, s)         # round half up = nearest: no tie
    # the constructed bases: every block of the factor-2 base is a tie; the others sit either side of one
    cell = M.BY_NAME["rs-ties"]
    b2, b3, b5 = (b[0] for b in M.cell_bases(cell))
    s2 = b2.reshape(8, 2, 12, 2).astype(np.int64).sum(axis=(1, 3))
    assert np.all(s2 % 4 == 2) and len(set(s2.ravel().tolist())) > 40
    assert np.array_equal(M.downscale_int_exact(b2, 2), s2 // 4 + 1) and np.array_equal(M.area_resize_exact(b2, 8, 12), s2 // 4 + 1)
    for b, f in ((b3, 3), (b5, 5)):
        s = b.reshape(8, f, 12, f).astype(np.int64).sum(axis=(1, 3))
        rem = s % (f * f)
        assert set(rem.ravel().tolist()) == {(f * f - 1) // 2, (f * f + 1) // 2}
        want = s // (f * f) + (rem > f * f // 2)
        assert np.array_equal(M.downscale_int_exact(b, f), want) and np.array_equal(M.area_resize_exact(b, 8, 12), want)


def test_saturated_and_zero_contents():
    sat, zero = (b[0] for b in M.cell_bases(M.BY_NAME["rs-sat-zero"]))
    assert sat.min() == 255 and zero.max() == 0
    for r in M.BY_NAME["rs-sat-zero"]["recs"]:
        s, z = M.apply_variant(sat, r), M.apply_variant(zero, r)
        assert s.shape == z.shape == M.unit_shape(sat.shape, r) and s.min() == 255 and z.max() == 0, r
    u16 = np.full((9, 9), 65535, np.uint16)
    for f in (2, 3, 5, 7):
        assert M.downscale_int_exact(u16, f).min() == 65535 and M.downscale_int_exact(u16, f).dtype == np.uint16


def test_masks_of_ones_and_of_255_under_both_resizes():
    """A 0 / 255 mask byte survives a resize wherever a 255 covers at least 1 / 510 of the footprint; a 0 / 1 byte only where
    the ones cover at least half of it - below that the area mean rounds to 0 and the mask is binarised to 0."""
    ones = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1]], np.uint8)
    assert M.downscale_int_exact(ones, 2).tolist() == [[1, 0], [0, 1]]                     # sums 3, 0, 0, 3: (s + 2) >> 2
    assert M.area_resize_exact(ones, 2, 2).tolist() == [[1, 0], [0, 1]]
    assert M.area_resize_exact(ones, 1, 1).tolist() == [[0]]                               # 6 / 16 < 1 / 2: binarised to 0
    assert M.downscale_int_exact(ones * 255, 2).tolist() == [[191, 0], [0, 191]]           # 765 / 4 = 191.25
    assert M.area_resize_exact(ones * 255, 1, 1).tolist() == [[96]]                        # 1530 / 16 = 95.625
    half = np.array([[1, 0], [0, 1]], np.uint8)
    assert M.area_resize_exact(half, 1, 1).tolist() == [[1]] and M.downscale_int_exact(half, 2).tolist() == [[1]]   # the tie: up
    assert M.area_resize_exact(half, 4, 4).tolist() == np.kron(half, np.ones((2, 2), np.uint8)).tolist()
    # the table's masks: the 0 / 1 ones lose area where they are sparse, the 0 / 255 ones keep it
    for name, top in (("rs-masks-01", 1), ("rs-masks-255", 255)):
        cell = M.BY_NAME[name]
        for px, mask in M.cell_bases(cell):
            assert set(np.unique(mask).tolist()) == {0, top}
            for r in cell["recs"]:
                if r[3] == 0:
                    small = M.apply_variant(mask, r)
                    f = r[5]
                    blocks = (mask[:small.shape[0] * f, :small.shape[1] * f] > 0).reshape(small.shape[0], f, small.shape[1], f).sum(axis=(1, 3))
                    if top == 1:
                        assert np.array_equal(small > 0, 2 * blocks >= f * f) and np.any((blocks > 0) & (small == 0)), (name, r)
                    else:
                        assert np.array_equal(small > 0, blocks > 0), (name, r)


# ---- views -----------------------------------------------------------------------------------------------------------------
def test_sixteen_records_are_the_eight_views():
    a = np.arange(15, dtype=np.uint8).reshape(3, 5)                         # non-square, no symmetry
    seen = {}
    for r in M.RECORDS16:
        k, lr, ud = r[:3]
        want = a
        if lr:
            want = np.fliplr(want)
        if ud:
            want = np.flipud(want)
        want = np.rot90(want, k)
        got = M.apply_variant(a, r)
        assert _eq(got, np.ascontiguousarray(want)), r
        seen.setdefault(got.shape + tuple(got.ravel().tolist()), []).append(r)
    assert len(seen) == 8 and all(len(v) == 2 for v in seen.values())
    assert len({M.view_of(r) for r in M.RECORDS16}) == 8 == len({M.view_of(r) for r in M.VIEWS8})
    # the eight, written out: rows of the 3 x 5 base as the view shows them
    t = a.T
    # (a quarter turn of a: new(i, j) = a(j, W - 1 - i) = t[::-1]; of the left-right mirror: a(j, i) = t)
    want8 = [a, a[:, ::-1], a[::-1], a[::-1, ::-1], t[::-1], t[:, ::-1], t, t[::-1, ::-1]]
    names = [M.rec(0), M.rec(0, 1, 0), M.rec(0, 0, 1), M.rec(2), M.rec(1), M.rec(3), M.rec(1, 1, 0), M.rec(1, 0, 1)]
    for r, w in zip(names, want8):
        assert _eq(M.apply_variant(a, r), np.ascontiguousarray(w)), r
    assert all(M.unit_shape((3, 5), r) == (3, 5) for r in M.EVEN_VIEWS) and all(M.unit_shape((3, 5), r) == (5, 3) for r in M.ODD_VIEWS)
    # a colour base turns its planes, not its channels
    rgb = np.arange(30, dtype=np.uint8).reshape(2, 5, 3)
    for r in M.RECORDS16:
        got = M.apply_variant(rgb, r)
        for c in range(3):
            assert _eq(got[:, :, c], M.apply_variant(np.ascontiguousarray(rgb[:, :, c]), r))


def test_expand_is_base_major():
    bases = [(np.full((2, 3), 10 * b, np.uint8), None) for b in range(3)]
    recs = (M.rec(0), M.rec(1), M.rec(0, down=2))
    units = M.expand(bases, recs)
    assert [(int(u[0][0, 0]), u[0].shape) for u in units] == [(10 * b, s) for b in range(3) for s in ((2, 3), (3, 2), (1, 1))]


# ---- the exactness premise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fb-dot4-views", "m-rgb-perchan", "rs-masks-01"])
def test_direct_sums_are_a_plain_triple_loop(name):
    """O.sliding_corr(..., force="direct") - the sums every epilogue of O.match_template(..., corr="direct") starts from -
    against Python-integer loops on the table's smallest cells, operand by operand as the oracle forms them (masked: I x T M
    and I^2 x M with the binarised mask)."""
    cell = M.BY_NAME[name]
    units = M.expand(M.cell_bases(cell), cell["recs"])
    img = M.cell_image(cell, units)
    small = min(range(len(units)), key=lambda i: units[i][0].size)
    for i in {small, len(units) - 1}:
        t, mask = units[i]
        a3, t3 = O._as3d(img).astype(np.float64), O._as3d(t).astype(np.float64)
        for c in range(a3.shape[2]):
            if mask is None:
                pairs = [(a3[:, :, c], t3[:, :, c])]
            else:
                m = (O._as3d(mask)[:, :, c] > 0).astype(np.float64)
                pairs = [(a3[:, :, c], t3[:, :, c] * m), (a3[:, :, c] ** 2, m)]
            for x, k in pairs:
                got = O.sliding_corr(x, k, exact_int=True, force="direct")
                assert got.dtype == np.float64 and np.array_equal(got, _triple_loop(x, k)), (name, i, c)


# ---- the table -------------------------------------------------------------------------------------------------------------
def _classes(cell):
    return [(m,) + c for m in cell["methods"] for c in M.cell_classes(cell, m)]


def test_hand_written_families_are_the_rule():
    for cell in M.CELLS:
        fams = {c[4]["family"] for c in _classes(cell)}
        if cell["want"]:
            assert fams == set(cell["want"]), (cell["name"], sorted(fams))
        for m, h, w, n, exp, views in _classes(cell):
            if (h, w) in cell["nt"]:
                assert exp["rm_nt"] == cell["nt"][(h, w)], (cell["name"], h, w, exp)
    # both sides of every doubling, as tests/test_gpu_tilings.py works them out
    assert [M.rm_group_templates(1, h, w) for h, w in ((31, 192), (32, 192), (12, 250), (13, 250), (31, 130), (32, 130))] == [1, 2, 1, 2, 1, 2]
    assert M.rm_group_templates(1, 70, 250) == 2 and M.rm_group_templates(3, 70, 250) == 4 and M.rm_group_templates(1, 258, 256) == 2
    # and the rule on the cells of that file's table whose expectation it states
    for n, h, w, chans, method, masked, fam in ((20, 24, 49, 1, 5, False, "r2_screen"), (20, 7, 64, 1, 3, False, "r2_noscreen"),
                                                (20, 72, 64, 1, 5, False, "r2_noscreen"), (20, 20, 40, 1, 0, False, "plain"),
                                                (20, 65, 192, 1, 3, False, "plain"), (20, 65, 40, 1, 5, False, "plain_kp"),
                                                (5, 259, 256, 1, 5, False, "plain"), (3, 148, 148, 3, 5, False, "rm_kp"),
                                                (3, 149, 148, 3, 3, False, "plain_kp"), (3, 172, 128, 3, 5, False, "rm"),
                                                (1, 511, 256, 1, 5, False, "plain"), (1, 512, 256, 1, 5, False, "slab_rm"),
                                                (20, 20, 257, 1, 3, False, "slab_plain"), (1, 258, 256, 1, 3, True, "rm"),
                                                (1, 259, 256, 1, 1, True, "off_cores"), (20, 24, 40, 1, 1, True, "plain_kp"),
                                                (3, 24, 40, 1, 3, True, "rm_kp"), (20, 24, 64, 1, 3, True, "plain"), (20, 20, 64, 1, 2, False, "r2_screen")):
        assert M.expected_tiling(n, h, w, chans, method, masked)["family"] == fam, (n, h, w, chans, method, masked)


def test_the_table_covers_what_it_is_there_for():
    cells = M.CELLS
    widths = {s[1] for c in cells for s in M.cell_units_shapes(c)}
    assert {w % 16 for w in widths} >= {15, 0, 1}
    by_family = {}
    for cell in cells:
        for m, h, w, n, exp, views in _classes(cell):
            by_family.setdefault(exp["family"], []).append((cell, h, w, n, exp, views))
    assert set(by_family) == set(M.FAMILIES)
    # every block count 1 .. 4 of a class that is not packed K, and packed K with every fill of the last MFMA step
    assert {(w + 63) // 64 for f in ("plain", "rm", "r2_screen", "r2_noscreen") for _, h, w, n, e, v in by_family[f]} >= {1, 2, 3, 4}
    assert {(w + 63) // 64 for _, h, w, n, e, v in by_family["plain"]} >= {1, 2, 4}
    assert {(h * e["kp_nseg"]) % 4 for _, h, w, n, e, v in by_family["plain_kp"]} == {0, 1, 2, 3}
    assert {w % 16 for _, h, w, n, e, v in by_family["plain_kp"]} >= {15, 0, 1}
    # every view at every family of the views x tilings sweep; a non-identity view at every other one
    for f in M.VIEW_FAMILIES:
        assert {v for *_, views in by_family[f] for v in views} == {M.view_of(r) for r in M.VIEWS8}, f
    for f in M.FAMILIES:
        assert any(v != M.IDENTITY for *_, views in by_family[f] for v in views), f
    # a quarter turn moves a class to another tiling
    assert any(len({c[4]["family"] for c in _classes(cell)}) == 2 for cell in cells if cell["group"] == "views")
    # both sides of the nt doublings, with one and with three units
    nts = {(n, h, w, e["rm_nt"]) for f in ("rm", "rm_kp") for _, h, w, n, e, v in by_family[f]}
    assert nts >= {(1, 31, 192, 1), (1, 32, 192, 2), (1, 12, 250, 1), (1, 13, 250, 2), (3, 31, 192, 4), (3, 13, 250, 4),
                   (1, 31, 130, 1), (1, 32, 130, 2)}
    # class sizes around the 16-unit groups
    for shape in ((24, 49), (9, 81)):
        assert {n for f in by_family.values() for c, h, w, n, e, v in f if c["group"] == "sizes" and (h, w) == shape} == {1, 15, 16, 17, 33}
    # resizes: both kinds, with and without a mask, one and three channels; every remainder under every factor
    kinds = {("sizes" if r[3] else "factors", bool(c["mask"]), c["chans"]) for c in cells for r in c["recs"] if r[3] or r[5] > 1}
    assert kinds >= {(k, m, 1) for k in ("sizes", "factors") for m in (False, True)} | {("sizes", False, 3), ("factors", False, 3), ("sizes", True, 3)}
    for f in M.FACTORS:
        assert {h % f for h, w in M.FACTOR_BASES} == set(range(f)) == {w % f for h, w in M.FACTOR_BASES}, f
        assert {M.IMAGE_DOWN_SHAPE[0] % f, M.IMAGE_DOWN_SHAPE[1] % f} != {0}
    rs = M.BY_NAME["rs-sizes"]
    shapes = {(b, (r[3], r[4])) for b in rs["bases"] for r in rs["recs"]}
    assert any(r[0] < b[0] and r[1] < b[1] and b[0] % r[0] for b, r in shapes) and any(r[0] > b[0] and r[1] > b[1] for b, r in shapes)
    assert any(r == (1, 1) for b, r in shapes) and any(r == b for b, r in shapes)
    assert any(r[0] > b[0] and r[1] < b[1] for b, r in shapes) and any(r[0] < b[0] and r[1] > b[1] for b, r in shapes)
    assert {(24, 49), (9, 81)} <= {r for b, r in shapes} and max(r[0] * r[1] for b, r in shapes) > 4 * 256
    full = [c for c in cells if c["methods"] == M.ALL_METHODS]
    assert len(full) >= 4 and {(c["chans"], bool(r[3])) for c in full for r in c["recs"]} == {(1, True), (1, False), (3, True), (3, False)}
    assert any(c["chans"] == 3 and c["mask"] and set(c["methods"]) == set(M.MASK_METHODS) for c in cells if c["group"] == "resize")
    # masks: four views of one shape as four classes; masked cells on every route the issue lists
    four = M.cell_classes(M.BY_NAME["m-four-views"], 3)
    assert len(four) == 4 and {(h, w, n) for h, w, n, e, v in four} == {(24, 40, 1)}
    assert len(M.cell_classes(M.BY_NAME["m-square-turns"], 3)) == 4 and len(M.cell_classes(M.BY_NAME["m-one-byte"], 3)) == 2
    a, b = (x[1] for x in M.cell_bases(M.BY_NAME["m-one-byte"]))
    assert int(np.count_nonzero(a != b)) == 1
    a, b = (x[1] for x in M.cell_bases(M.BY_NAME["m-identical"]))
    assert np.array_equal(a, b)
    masked = {e["family"] for c in cells if c["mask"] for m, h, w, n, e, v in _classes(c)}
    assert masked >= {"plain", "plain_kp", "rm", "rm_kp", "off_cores", "naive"}
    for cell in cells:                                                    # an asymmetric mask: its eight views all differ
        if cell["mask"] in ("asym", "same", "asym01"):
            m = M.cell_bases(cell)[0][1]
            assert len({(M.unit_shape(m.shape, r), M.apply_variant(m, r).tobytes()) for r in M.VIEWS8}) == 8, cell["name"]
    # images stay small
    for cell in cells:
        shapes = M.cell_units_shapes(cell)
        assert max(s[0] for s in shapes) + 12 <= 530 and max(s[1] for s in shapes) + 37 <= 300, cell["name"]
