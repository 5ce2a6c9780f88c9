"""The frames of tests/front_cases.py reach the edges they are named after, and tests/front_ref.py, the plain NumPy statement
of S0-S3, equals the CPU oracle on every one of them and on a few hundred seeded random frames (no GPU needed).  The GPU
tests (test_gpu_front.py) rely on both.

Which cases notice a broken rule, measured on scratch copies of the oracle with one rule broken each (the comparison
front_ref against oracle of the `staged` fixture names the first of them; the known answers below hold either side alone):
  column sw - 1 initiating links (join mask)   "border columns, black" (the right bar's pixels join through "up" and "left"
                                               instead of staying alone), "last column, sw = *", and every frame with a
                                               coloured last column: 108 of the 133 cases
  diagonals for black too                      "contact: black up-left / up-right, *" (the two blobs merge), and every frame
                                               whose last column is black: 102 cases
  the contrast floor, < 4 instead of < 5       "floor: 104 on 100, *" alone
  the contrast floor, < 6                      "floor: 105 on 100, *" and "cut: 252, *"
  leftover pixels not given the nearest tile   "leftover *: beside a tile with contrast", "last column, sw = 65 / 66",
                                               "border columns, *", "batch: *" (130 wide): 40 cases
"""
import numpy as np
import pytest

import front_cases as F
import front_ref as R
import oracle_lib as O


def _oracle_front(frame, f):
    g = O.decimate(O.bgr2gray(frame) if frame.ndim == 3 else frame, f)
    th = O.threshold(g)
    lab, sz = O.connected_components(th)
    return g, th, lab, sz


def _same(frame, f, name):
    """front_ref == oracle for all four products; returns the oracle's"""
    mine, ref = R.front(frame, f), _oracle_front(frame, f)
    for what, a, b in zip(("gray", "threshold", "labels"), mine, ref):
        assert a.shape == b.shape and np.array_equal(a, b), (name, what)
    roots = ref[2].ravel() == np.arange(ref[2].size)
    assert np.array_equal(mine[3].ravel()[roots], ref[3].ravel()[roots]), (name, "sizes")
    assert not mine[3].ravel()[~roots].any(), name
    return ref


@pytest.fixture(scope="module")
def staged():
    """name -> (case, the oracle's gray, threshold, labels, sizes), front_ref held equal; computed once"""
    cases = (F.decimation() + F.corner_colours() + F.smallest_frames() + F.contrast_floor() + F.dilation_reach() + F.leftovers() +
             F.segments() + F.drawn() + F.capacity())
    out = {c["name"]: (c, _same(c["frame"], c["f"], c["name"])) for c in cases}
    assert len(out) == len(cases)  # the names are unique
    return out


def _group(staged, cases):
    return [staged[c["name"]] for c in cases]


def _components(th, colour):
    """{label: size} of the components of one colour, front_ref's"""
    lab, sz = R.components(th)
    return {int(l): int(sz.ravel()[l]) for l in np.unique(lab[th == colour])}


# ------------------------------------------------------------------------------------------------------------------------- A
def test_front_ref_equals_the_oracle_on_random_frames():
    """300 seeded frames, sizes 8 .. 140, all five factors, gray and BGR; every third one a salted two-level texture so that
    large components occur too."""
    rng = np.random.default_rng(2024)
    for k in range(300):
        w, h = int(rng.integers(8, 141)), int(rng.integers(8, 141))
        f = F.FACTORS[k % 5]
        if k % 3 == 0:
            frame = np.where(rng.random((h, w)) < rng.uniform(0.2, 0.8), F.LIGHT, F.DARK).astype(np.uint8)
        elif k % 3 == 1:
            frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        else:
            frame = (rng.integers(0, 256, (h // 4 + 1, w // 4 + 1), dtype=np.uint8).repeat(4, axis=0).repeat(4, axis=1)[:h, :w] // 64 * 64 +
                     rng.integers(0, 6, (h, w), dtype=np.uint8)).astype(np.uint8)
        _same(frame, f, "random %d: %dx%d decimate %d" % (k, w, h, f))


def test_decimation_sizes_cover_every_residue(staged):
    for f in (2, 3):
        mine = [c for c in F.decimation() if c["f"] == f]
        assert {c["dec"][0] % 4 for c in mine} == {0, 1, 2, 3} == {c["dec"][1] % 4 for c in mine}
        assert any(c["frame"].shape[1] % f for c in mine) and any(c["frame"].shape[0] % f for c in mine)
        assert {c["frame"].ndim for c in mine} == {2, 3}
    assert {c["f"] for c in F.decimation()} == set(F.FACTORS)
    for c, (g, th, lab, sz) in _group(staged, F.decimation() + F.smallest_frames()):
        assert g.shape == c["dec"][::-1], c["name"]


def test_corner_colours_hit_both_ends_of_the_fixed_point(staged):
    c, (g, th, lab, sz) = staged["corner colours, decimate 1"]
    assert sorted(set(g.ravel().tolist())) == sorted({0, 29, 150, 179, 76, 105, 226, 255})  # 0.114, 0.587, 0.299 of 255, rounded, and their sums


def test_padding_bytes_would_show():
    for name, f, ch, frames in F.padded_layouts():
        buf, stride, pitch = F.pad_batch(frames, ch)
        B, h, w = frames.shape[:3]
        assert stride == w * ch + 5 and pitch == stride * h + 11 and len(buf) == B * pitch
        assert len({fr.tobytes() for fr in frames}) == 3
        own = np.zeros(len(buf), bool)
        for b in range(B):
            rows = buf[b * pitch:b * pitch + stride * h].reshape(h, stride)
            assert np.array_equal(rows[:, :w * ch].reshape(frames[b].shape), frames[b])
            own[b * pitch:b * pitch + stride * h].reshape(h, stride)[:, :w * ch] = True
        pad = buf[~own]
        assert set(pad.tolist()) == {0, 255} and (pad == 0).sum() > len(pad) // 3 and (pad == 255).sum() > len(pad) // 3, name


def test_smallest_frames_are_what_the_oracle_gives(staged):
    for c, (g, th, lab, sz) in _group(staged, F.smallest_frames()):
        s = c["dec"][0]
        if s < 4:
            assert (th == 127).all() and th.shape == (s, s) and s in (1, 2, 3), c["name"]
            assert np.array_equal(lab.ravel(), np.arange(s * s)), c["name"]
    assert {c["dec"][0] for c in F.smallest_frames()} == {8, 4, 3, 1, 2}


# ------------------------------------------------------------------------------------------------------------------------- B
def test_contrast_floor_and_cut_known_answers(staged):
    for c, (g, th, lab, sz) in _group(staged, F.contrast_floor() + F.leftovers()):
        assert (th == 127).all() == c["blank"], c["name"]
        for (x, y), v in c["expect"]:
            assert th[y, x] == v, (c["name"], (x, y), int(th[y, x]), v)
    for sw in (32, 36):
        c, (g, th, lab, sz) = staged["cut: 252, %d wide" % sw]
        lo, hi = R.tile_cuts(g)
        assert (lo + (hi - lo) // 2).max() == 252 and g.shape[1] // 4 % 4 == (0 if sw == 32 else 1)
    assert {(sw % 4, sh % 4) for sw, sh in F.LEFTOVER_SIZES} == {(1, 1), (2, 2), (3, 3)}


def test_dilation_reaches_exactly_the_neighbouring_tiles(staged):
    seen_tw, seen_at = set(), set()
    for c, (g, th, lab, sz) in _group(staged, F.dilation_reach()):
        x0, y0, x1, y1 = c["box"]
        inside = np.zeros(th.shape, bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        assert np.array_equal(th != 127, inside), c["name"]
        assert (th == 255).sum() == 1, c["name"]
        tw, thh = c["tiles"]
        seen_tw.add((tw % 4, c["at"][0] == tw - 1))
        seen_at.add((tw, thh, c["at"]))
    assert {(r, True) for r in range(4)} <= seen_tw  # the last tile column for every tw mod 4
    assert {(9, 9, p) for p in ((0, 0), (8, 0), (0, 8), (8, 8), (3, 1), (4, 1), (1, 3), (1, 4))} <= seen_at
    assert any(tw == 4 for tw, _, _ in seen_at) and any(tw < 4 for tw, _, _ in seen_at) and any(t < 4 for _, t, _ in seen_at)
    assert any(t % 4 for _, t, _ in seen_at)


def test_segment_sizes_and_their_launches(staged):
    assert {sw % 16 for sw, sh in F.SEGMENT_SIZES} >= {0, 1, 15} and {sw % 64 for sw, sh in F.SEGMENT_SIZES} >= {0, 1, 63}
    assert {sh % 32 for sw, sh in F.SEGMENT_SIZES} >= {0, 1, 17, 31}
    for c, (g, th, lab, sz) in _group(staged, F.segments()):
        assert (th[:, -1] != 127).any() and (th[-1] != 127).any(), c["name"]
        n = F.dense_tiles(th)
        print(c["name"], "dense labelling tiles:", n, "of", len(F.tile_counts(th)))
        if c["kind"] == "blocks":
            assert n == 0, c["name"]
        elif th.shape[1] >= 63 and th.shape[0] >= 31:
            assert n >= 1, c["name"]


# ------------------------------------------------------------------------------------------------------------------------- C
def test_drawn_frames_threshold_to_their_drawing(staged):
    for c, (g, th, lab, sz) in _group(staged, F.drawn() + F.capacity()):
        assert set(np.unique(c["frame"]).tolist()) == {F.DARK, F.LIGHT}, c["name"]
        assert np.array_equal(th, F.binary(c["frame"])), c["name"]
    for c, (g, th, lab, sz) in _group(staged, F.drawn()):
        assert F.dense_tiles(th) == 0, c["name"]


def _side(cells, axis, s):
    v = [p[axis] for p in cells]
    return max(v) < s or min(v) >= s


def test_single_contacts_are_the_only_contact(staged):
    cases = F.single_contacts()
    assert len(cases) == 2 * 16
    for c, (g, th, lab, sz) in _group(staged, cases):
        v = 255 if c["white"] else 0
        A, B, a, b = c["A"], c["B"], c["a"], c["b"]
        assert len(set(A)) >= 25 and len(set(B)) >= 25 and not set(A) & set(B), c["name"]
        assert all(th[y, x] == v for x, y in A + B)
        la, lb = int(lab[a[1], a[0]]), int(lab[b[1], b[0]])
        inA, inB = {(int(x), int(y)) for y, x in zip(*np.nonzero(lab == la))}, {(int(x), int(y)) for y, x in zip(*np.nonzero(lab == lb))}
        if c["merges"]:
            assert la == lb and inA == set(A) | set(B) and sz[lab == la][0] == len(set(A)) + len(set(B)), c["name"]
        else:
            assert la != lb and inA == set(A) and inB == set(B), c["name"]
        # without either pixel of the pair the blobs are apart
        for p in (a, b):
            g2 = c["frame"].copy()
            g2[p[1], p[0]] = F.DARK if c["white"] else F.LIGHT
            lab2, _ = R.components(F.binary(g2))
            qa, qb = (A[1], b) if p == a else (a, B[1])
            assert lab2[qa[1], qa[0]] != lab2[qb[1], qb[0]], c["name"]
        # each blob lies wholly on its side of the seam the pair is placed on
        place = c["place"]
        if "word seam" in place or "corner" in place:
            if c["kind"] != "v":
                assert _side(A, 0, 64) and _side(B, 0, 64) and (a[0] < 64) != (b[0] < 64), c["name"]
        if "row seam" in place or "corner" in place:
            if c["kind"] != "h":
                assert _side(A, 1, 32) and _side(B, 1, 32) and (a[1] < 32) != (b[1] < 32), c["name"]
        if place == "inside":
            cells = A[:1] + B[:1]
            assert len({x // 64 for x, y in cells}) == 1 and len({y // 32 for x, y in cells}) == 1
    corners = {(c["a"], c["b"]) for c in cases if c["place"] == "corner"}
    assert corners == {((63, 31), (64, 32)), ((64, 31), (63, 32))}


def test_last_column_joins_through_the_diagonal_alone(staged):
    for c, (g, th, lab, sz) in _group(staged, F.last_column()):
        for sw, y in c["sites"]:
            assert th.shape[1] == sw
            assert th[y, sw - 2] == th[y - 1, sw - 2] == th[y - 1, sw - 1] == 255 and th[y, sw - 1] == 0
            l = int(lab[y, sw - 2])
            assert lab[y - 1, sw - 1] == l and sz.ravel()[l] == 8, c["name"]
            g2 = c["frame"].copy()
            g2[y, sw - 2] = F.DARK  # the pixel that holds the diagonal: without it pixel sw - 1 is alone
            lab2, sz2 = R.components(F.binary(g2))
            assert sz2[y - 1, sw - 1] == 1, c["name"]


def test_border_columns_known_answers(staged):
    for c, (g, th, lab, sz) in _group(staged, F.border_columns()):
        v, sw = (255 if c["white"] else 0), th.shape[1]
        bars = [(x, y) for x in (0, sw - 1) for y in F.BAR_ROWS]
        assert all(th[y, x] == v for x, y in bars)
        grouped = set().union(*c["groups"])
        for grp in c["groups"]:
            ls = {int(lab[y, x]) for x, y in grp}
            assert len(ls) == 1 and int((lab == ls.pop()).sum()) == len(grp), (c["name"], grp)
        alone = [p for p in bars if p not in grouped]
        assert all(sz[y, x] == 1 and lab[y, x] == y * sw + x for x, y in alone), c["name"]
        assert len(alone) == (80 - 4 if c["white"] else 80 - 2)
        if not c["white"]:
            assert th[21, sw - 2] == 0 and sz[21, sw - 2] == 1  # beside the last column, and still alone


def test_long_components_known_answers(staged):
    for c, (g, th, lab, sz) in _group(staged, F.long_components()):
        assert th.shape == (96, 192)
        for colour, (size, root) in ((255, c["white"]), (0, c["black"])):
            big = {l: n for l, n in _components(th, colour).items() if n > 1}
            assert big == {root: size}, (c["name"], colour, big)
            assert sz.ravel()[root] == size and (lab[th == colour] == root).sum() == size
        cols = np.nonzero((lab == c["white"][1]).any(axis=0))[0]
        rows = np.nonzero((lab == c["white"][1]).any(axis=1))[0]
        assert cols.min() < 64 and cols.max() >= 128 and rows.min() < 32 and rows.max() >= 64  # all nine tiles' words and row blocks
    # a comb's teeth are apart until the spine: every tile above (below) it holds a root per tooth
    for name, spine in (("comb", 93), ("comb, mirrored", 2)):
        c, (g, th, lab, sz) = staged[name]
        cut = c["frame"].copy()
        cut[spine] = F.DARK
        teeth = {l: n for l, n in _components(F.binary(cut), 255).items() if n > 1}
        assert len(teeth) == 13 and set(teeth.values()) == {91}, (name, teeth)  # 6 + 6 + 1 teeth of rows 2 .. 92


def test_seam_pair_frames(staged):
    for c, (g, th, lab, sz) in _group(staged, F.seam_pairs() + F.label_batch()):
        pair = (th[:, 63] == th[:, 64]) & (th[:, 63] != 127)
        assert pair[2:th.shape[0] - 2].all() or "stairs" in c["name"], c["name"]  # a link across seam 64 in every row of the feature
        keys = [(int(lab[y, 63]), int(th[y, 63])) for y in range(2, th.shape[0] - 2)]
        same = sum(1 for k0, k1 in zip(keys, keys[1:]) if k0 == k1)
        if "band" in c["name"]:
            assert same == len(keys) - 1, c["name"]
        elif "rungs" in c["name"]:
            assert len({k for k in keys if k[1] == 255}) == len(keys) // 2 and same == 0, c["name"]
        else:
            white = [k for k in keys if k[1] == 255]
            assert len(set(white)) >= (5 if "seam pairs" in c["name"] else 2) and any(k0 == k1 and k0[1] == 255 for k0, k1 in zip(keys, keys[1:])), c["name"]
    frames = [c["frame"] for c in F.label_batch()]
    assert len(frames) >= 3 and {f.shape for f in frames} == {(40, 130)} and len({f.tobytes() for f in frames}) == len(frames)
    for f in frames:
        assert (F.binary(f)[:, 129] == 255).any() and (F.binary(f)[:, 127] == F.binary(f)[:, 128]).any()


def test_capacity_tiles_hold_exactly_what_they_are_named_after(staged):
    for c, (g, th, lab, sz) in _group(staged, F.capacity()):
        counts = F.tile_counts(th)
        runs, nlinks = counts[F.CAP_TILE]
        print(c["name"], "runs, links of every tile:", counts)
        if c["what"] == "runs":
            assert runs == c["target"] and nlinks < F.SEG_CAP, (c["name"], runs, nlinks)
        else:
            assert nlinks == c["target"] and runs < F.SEG_CAP, (c["name"], runs, nlinks)
        assert F.dense_tiles(th) == c["dense"] == (1 if c["target"] > F.SEG_CAP else 0)
        assert all(r < F.SEG_CAP // 2 and l < F.SEG_CAP // 2 for k, (r, l) in counts.items() if k != F.CAP_TILE)  # ordinary tiles around it
        # components that cross from the tile under test into the tiles on its left, on its right and below
        line = lab == lab[20, 100]
        assert th[20, 100] == 255 and line[:, :64].any() and line[:, 128:].any() and line[32:].any() and line[:32, 64:128].any(), c["name"]
        ground = lab == lab[31, 127]
        assert th[31, 127] == 0 and ground[:, :64].any() and ground[:, 128:].any() and ground[32:].any(), c["name"]
    assert [(c["what"], c["target"]) for c in F.capacity()] == [("runs", 511), ("runs", 512), ("runs", 513), ("links", 512), ("links", 513)]


def test_run_and_link_counts_agree_with_the_definition():
    """tile_counts against a direct count on a random two-level image: runs are maximal stretches of one colour inside a word
    whose pixels after the first may initiate links; every link of front_ref.links() that stays inside a tile is counted
    once per pair of touching stretches at most (links <= definition's) and no tile without a link reports one."""
    # known answer: a row W.W.W... above an all-white row, in a word that has neighbours on both sides -- the lower row is
    # one run with 32 links up, 32 up-left and 31 up-right (bit 63's goes to the next word: k_seg_border's)
    th = np.zeros((2, 192), np.uint8)
    th[0, 64:128:2] = 255
    th[1, 64:128] = 255
    assert F.tile_counts(th)[(1, 0)] == (32 + 32 + 1 + 0, 95)  # row 0: 32 white and 32 black runs; row 1: one white run
    rng = np.random.default_rng(7)
    th = np.where(rng.random((70, 150)) < 0.5, 255, 0).astype(np.uint8)
    th[rng.random(th.shape) < 0.1] = 127
    counts = F.tile_counts(th)
    sh, sw = th.shape
    for (wx, ty), (runs, nlinks) in counts.items():
        n = 0
        for y in range(ty * 32, min(ty * 32 + 32, sh)):
            for x in range(wx * 64, min(wx * 64 + 64, sw)):
                if th[y, x] != 127 and (x == wx * 64 or th[y, x - 1] != th[y, x] or not 1 <= x <= sw - 2):
                    n += 1
        assert runs == n, (wx, ty)
    a, b = R.links(th)
    inside = ((a // sw) // 32 == (b // sw) // 32) & ((a % sw) // 64 == (b % sw) // 64) & (a // sw != b // sw)
    for (wx, ty), (runs, nlinks) in counts.items():
        mine = int((inside & ((a // sw) // 32 == ty) & ((a % sw) // 64 == wx)).sum())
        assert 0 < nlinks <= mine, (wx, ty, nlinks, mine)
