"""Copy-paste of tiny objects without a GPU (crops.py: ObjectPaste; tests/paste_oracle.py): constructor validation, the
source table on a planted scene, the invariants of the draw over 200 windows, what the input sets of
tests/test_gpu_paste.py are there for, and planted mutations: each bends one rule of a copy of the restatement, and the
comparison the GPU test makes against the restatement must fail for it on those input sets.

Mutation 7 of the issue's list (the merge storing where v == t) is dropped as unobservable: a store of v where v == t
writes the bits that are there (v is never -0.0 and a NaN is equal to nothing), so no comparison of results can see
it; test_merge_on_a_tie_is_unobservable shows exactly that -- the rule's written-elements mask differs, the target
does not."""
import numpy as np
import pytest
import torch

from tests import paste_oracle as po


# ---------------------------------------------------------------------------------------------------------------
def test_constructor_validation():
    from unet_nested4tiny_objects_keypoints_amd import ObjectPaste
    ps = ObjectPaste()
    assert (ps.max_pastes, ps.p, ps.patch_radius, ps.core, ps.clearance, ps.dihedral) == (4, 0.5, 4, 2.5, 8.0, True)
    assert ObjectPaste(patch_radius=2, core=1.0, clearance=3.5).clearance == 3.5
    for bad in (dict(max_pastes=0), dict(max_pastes=65), dict(max_pastes=2.0), dict(max_pastes=True), dict(p=-0.1),
                dict(p=1.5), dict(p=float("nan")), dict(patch_radius=-1), dict(patch_radius=17), dict(patch_radius=1.0),
                dict(core=4.5), dict(core=-1.0), dict(core=float("nan")), dict(patch_radius=1, core=1.5),
                dict(clearance=-1.0), dict(clearance=float("nan")), dict(clearance=float("inf"))):
        with pytest.raises(ValueError):
            ObjectPaste(**bad)
    with pytest.raises(ValueError):
        ps.set_sources([0], [[5.0, 5.0]], [0])                 # not yet given to a SceneCrops


def test_alpha_table():
    from unet_nested4tiny_objects_keypoints_amd.crops import paste_alpha
    for R, core in ((4, 2.5), (1, 0.6), (4, 2.4), (1, 1.49), (16, 3.0), (0, 0.25)):
        a = paste_alpha(R, core).numpy()
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), po.alpha_ref(R, core).view(np.int32)), (R, core)
        for sym in (a.T, a[::-1], a[:, ::-1], np.rot90(a)):    # symmetric under the eight codes
            assert np.array_equal(a, sym)
        assert a[R, R] == 1.0 and a.min() >= 0.0 and a.max() <= 1.0
    a = po.alpha_ref(4, 2.5)
    assert a[4, 6] == 1.0 and a[4, 7] == np.float32(0.75) and a[0, 0] == 0.0 and a[4, 8] == np.float32(0.25)
    assert (po.alpha_ref(1, 1.49) == 1.0).all()                # core just under R + 0.5 with R = 1: the whole patch


def test_source_table_on_a_planted_scene():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions
    from unet_nested4tiny_objects_keypoints_amd.crops import paste_source_table
    R, C, size = 3, 2, (60, 80)
    plant = [
        ((40.25, 30.5), 0, True),       # 0  the control: alone, inside
        ((10.0, 10.0), 1, False),       # 1  a neighbour at Chebyshev distance R + 1 = 4 ...
        ((14.0, 9.0), 0, False),        # 2  ... which sees label 1 at distance 4 from its own centre as well
        ((60.0, 10.0), 0, True),        # 3  a neighbour at R + 2 = 5: admitted ...
        ((65.0, 12.0), 1, True),        # 4  ... and so is the neighbour
        ((R - 1.0, 30.0), 0, False),    # 5  R - 1 from the left edge
        ((40.0, 60 - R + 0.0), 1, False),   # 6  R - 1 from the bottom edge (cy = Hs - R)
        ((70.0, 45.0), 0, False),       # 7  inside an ignore rectangle
        ((20.0, 45.0), C, False),       # 8  a class outside [0, C)
        ((-1.0, -1.0), 0, False),       # 9  a sentinel
        ((30.4, 50.0), -1, False),      # 10 class -1
    ]
    labels = np.array([[p for p, _, _ in plant], [(40.0, 30.0)] + [(-1.0, -1.0)] * (len(plant) - 1)], dtype=np.float32)
    classes = np.array([[c for _, c, _ in plant], [1] + [-1] * (len(plant) - 1)], dtype=np.int32)
    rects = np.array([[[68.0, 43.0, 72.0, 47.0]], [[0.0, 0.0, -1.0, -1.0]]], dtype=np.float32)   # frame 1: padding
    want_rows = [l for l, (_, _, ok) in enumerate(plant) if ok]
    ref = po.source_table_ref(labels, classes, C, size, R, rects, np.full((2, 1), -1))
    got = paste_source_table(torch.from_numpy(labels), torch.from_numpy(classes), C, size, R,
                             IgnoreRegions(torch.from_numpy(rects)))
    for g, r in zip(got, ref):
        assert g.dtype in (torch.int32, torch.float32) and np.array_equal(g.numpy(), r)
    frame, xy, cls = ref
    assert frame.tolist() == [0] * len(want_rows) + [1]
    assert np.array_equal(xy[:-1], labels[0, want_rows]) and cls.tolist() == [plant[l][1] for l in want_rows] + [1]
    # without the rectangle label 7 is admitted; a rectangle of a class outside [0, C) is padding
    assert len(po.source_table_ref(labels, classes, C, size, R)[0]) == len(want_rows) + 2
    assert len(po.source_table_ref(labels, classes, C, size, R, rects, np.full((2, 1), C))[0]) == len(want_rows) + 2
    got = paste_source_table(torch.from_numpy(labels), torch.from_numpy(classes), C, size, R,
                             IgnoreRegions(torch.from_numpy(rects), torch.full((2, 1), C)))
    assert got[0].numel() == len(want_rows) + 2


# ---------------------------------------------------------------------------------------------------------------
def test_draw_invariants_over_200_windows():
    rng = np.random.default_rng(5)
    N, K, R, C, M, L = 200, 6, 3, 3, 2, 40
    Ho, Wo = 40, 48
    clearance = 5.0
    labels = np.stack([rng.uniform(0, po.WS, (M, L)), rng.uniform(0, po.HS, (M, L))], axis=-1).astype(np.float32)
    classes = rng.integers(-1, C + 1, (M, L)).astype(np.int32)
    frame, xy, cls = po.source_table_ref(labels, classes, C, (po.HS, po.WS), R)
    assert len(frame) >= 5
    kinds = ("identity", "flip", "flip_y", "quarter", "three_quarters", "general")
    rows = np.stack([po.io.window_row(kinds[n % 6], (int(rng.integers(0, 60)), int(rng.integers(0, 40))), (Ho, Wo))
                     for n in range(N)]).astype(np.float32)
    index = rng.integers(0, M, N)
    index[::17] = -1
    d = po.Paste().draw(N, K, 99, frame, xy, cls, labels, classes, index, rows, C, (po.HS, po.WS), (Ho, Wo), 0.8, R, clearance)
    acc = d["src"] >= 0
    assert 100 < acc.sum() < N * K and not acc[::17].any()
    assert ((d["dst"][..., 0] >= R) & (d["dst"][..., 0] <= Wo - 1 - R)).all()             # inside the window, void or not
    assert ((d["dst"][..., 1] >= R) & (d["dst"][..., 1] <= Ho - 1 - R)).all()
    assert (d["cls"][~acc] == -1).all() and (d["xy"][~acc] == -1).all()                   # void slots carry class -1
    assert np.array_equal(d["cls"][acc], cls[d["src"][acc]])
    assert set(d["code"][acc].tolist()) == set(range(8))
    assert np.abs(d["xy"][acc] - d["dst"][acc]).max() <= 0.5
    for n in range(N):
        took = np.flatnonzero(acc[n])
        for a in took:
            for b in took:
                if a < b:                                                                 # pairwise disjoint patches
                    assert np.abs(d["dst"][n, a] - d["dst"][n, b]).max() > 2 * R, (n, a, b)
        if took.size:
            ok = (classes[index[n]] >= 0)
            xo, yo = po.co.window_positions(labels[index[n]], rows[n])
            for a in took:                                                                # no frame label within the clearance
                d2 = (xo[ok].astype(np.float64) - d["dst"][n, a, 0]) ** 2 + (yo[ok].astype(np.float64) - d["dst"][n, a, 1]) ** 2
                assert d2.min() >= clearance ** 2
    off = po.Paste().draw(N, K, 99, frame, xy, cls, labels, classes, index, rows, C, (po.HS, po.WS), (Ho, Wo), 0.0, R, clearance)
    assert not (off["src"] >= 0).any() and np.array_equal(off["dst"], d["dst"])
    plain = po.Paste().draw(N, K, 99, frame, xy, cls, labels, classes, index, rows, C, (po.HS, po.WS), (Ho, Wo), 0.8, R,
                            clearance, dihedral=False)
    assert not plain["code"].any()


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets():
    """every input set of the GPU test with the restatement's results: computed once, read by all"""
    out = {}
    for name in po.CASES:
        cs = po.case(name)
        rows = po.draw_of(cs)
        out[name] = (cs, rows, po.apply_of(cs, rows))
    return out


def test_the_input_sets_hold_what_they_are_there_for(sets):
    codes = set()
    for name, (cs, rows, pasted) in sets.items():
        acc = rows["src"] >= 0
        codes |= set(rows["code"][acc].tolist())
        if cs["K"] == 4:                                      # p = 1, K = 4: some accepted, some void
            assert acc.sum() >= 1 and (~acc).sum() >= 1, name
        if cs["N"] == 3:
            assert not acc[1].any()                           # index -1
        bad_rows = np.isin(np.arange(12), (8, 9, 10, 11))
        assert not np.isin(rows["src"][acc], np.flatnonzero(bad_rows)).any()
        changed = (pasted != cs["inputs"]).any(axis=1)        # the pixels that changed lie in accepted patches
        R = cs["R"]
        for n in range(cs["N"]):
            box = np.zeros(changed.shape[1:], dtype=bool)
            for k in np.flatnonzero(acc[n]):
                px, py = rows["dst"][n, k]
                box[py - R:py + R + 1, px - R:px + R + 1] = True
            assert not (changed[n] & ~box).any() and (changed[n].any() == acc[n].any())
    assert codes == set(range(8))
    assert any(cs["planted"] for cs, _, _ in sets.values())
    drawn = set()                                             # every kind of unusable source row was drawn somewhere
    for cs, _, _ in sets.values():
        for n in range(cs["N"]):
            for k in range(cs["K"]):
                drawn.add(po._pick(po.uniform(cs["seed"], n, k, 1), 12))
    assert {8, 9, 10, 11} <= drawn


def _same_rows(a, b):
    """the comparison of the GPU test's draw check: all five outputs bit for bit"""
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in ("src", "dst", "code", "xy", "cls"))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


class ForwardCodeOnPixels(po.Paste):                          # 1
    def pixel_offset(self, code, i, j):
        return self.label_offset(code, i, j)


class LabelOffsetNotTransformed(po.Paste):                    # 2
    def label_offset(self, code, ox, oy):
        return ox, oy


class GainOfWindowZero(po.Paste):                             # 3
    def gain_bias(self, rows, n):
        return po.Paste.gain_bias(self, rows, 0)


class ClearanceInclusive(po.Paste):                           # 4
    def too_close(self, d2, clearance2):
        return d2 <= clearance2


class OverlapStrict(po.Paste):                                # 5
    def overlaps(self, cheb, R):
        return cheb < 2 * R


class MergeOverwritesNegatives(po.Paste):                     # 6
    def keeps(self, t):
        return np.zeros(np.shape(t), dtype=bool)


class MergeStoresOnATie(po.Paste):                            # 7
    def stores(self, v, t):
        return v >= t


class ChannelZeroCoefficients(po.Paste):                      # 8
    def channel(self, mul, add, c):
        return po.Paste.channel(self, mul, add, 0)


def test_unmutated_restatement_passes_its_own_comparisons(sets):
    for name, (cs, rows, pasted) in sets.items():
        assert _same_rows(rows, po.draw_of(cs)) and _same_bits(pasted, po.apply_of(cs, rows)), name


@pytest.mark.parametrize("mutant", [LabelOffsetNotTransformed, ClearanceInclusive, OverlapStrict])
def test_draw_mutations_are_seen(sets, mutant):
    seen = [name for name, (cs, rows, _) in sets.items() if not _same_rows(rows, po.draw_of(cs, mutant()))]
    print(mutant.__name__, "seen in", seen)
    assert seen
    if mutant is ClearanceInclusive:                          # wherever a label was planted at exactly the clearance
        assert set(seen) >= {name for name, (cs, _, _) in sets.items() if cs["planted"]}


@pytest.mark.parametrize("mutant", [ForwardCodeOnPixels, GainOfWindowZero, ChannelZeroCoefficients])
def test_pixel_mutations_are_seen(sets, mutant):
    seen = [name for name, (cs, rows, pasted) in sets.items() if not _same_bits(pasted, po.apply_of(cs, rows, mutant()))]
    print(mutant.__name__, "seen in", seen)
    assert seen
    if mutant is ChannelZeroCoefficients:
        assert all(sets[name][0]["Cin"] == 3 for name in seen)


def _premarked(cs, rows):
    """the target the GPU test merges into: the frame's own target with the ignore marks on it"""
    base = po.co.points_target_ref(cs["labels"], cs["label_class"], cs["index"], cs["rows"], cs["C"],
                                   (cs["Ho"], cs["Wo"]), po.RADIUS)
    _, _, mask = po.ignore_rects(cs)
    return po.io.apply_mark(base, mask), mask


def test_merge_mutations(sets):
    seen6 = []
    for name, (cs, rows, _) in sets.items():
        marked, mask = _premarked(cs, rows)
        want, wrote = po.Paste().merge(marked, rows["xy"], rows["cls"], po.RADIUS)
        assert np.array_equal(want[mask], marked[mask]) and not wrote[mask].any()       # negatives preserved
        union, m_frame, m_paste = po.union_target_ref(cs["labels"], cs["label_class"], cs["index"], cs["rows"], cs["C"],
                                                      (cs["Ho"], cs["Wo"]), po.RADIUS, rows["xy"], rows["cls"])
        assert _same_bits(want[~mask], union[~mask]), name      # the merge of the restatement IS the union target
        assert _same_bits(want[m_frame < m_paste], marked[m_frame < m_paste])
        got, _ = MergeOverwritesNegatives().merge(marked, rows["xy"], rows["cls"], po.RADIUS)
        if not np.array_equal(got[mask], marked[mask]):         # the GPU test's comparison: negatives are preserved
            seen6.append(name)
    print("MergeOverwritesNegatives seen in", seen6)
    assert seen6


def test_merge_on_a_tie_is_unobservable(sets):
    ties = 0
    for name, (cs, rows, _) in sets.items():
        marked, _ = _premarked(cs, rows)
        want, wrote = po.Paste().merge(marked, rows["xy"], rows["cls"], po.RADIUS)
        again, wrote2 = po.Paste().merge(want, rows["xy"], rows["cls"], po.RADIUS)       # every stored element is now a tie
        assert _same_bits(again, want) and not wrote2.any()
        got, wrote7 = MergeStoresOnATie().merge(want, rows["xy"], rows["cls"], po.RADIUS)
        ties += int(wrote7.sum())
        assert _same_bits(got, want), name                      # the same target, bit for bit ...
    assert ties > 0                                             # ... though the rule stored: only a mask of writes shows it
