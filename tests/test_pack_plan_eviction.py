"""ops.PackPlan drops weight images that no pass used for a while.  A pass that records the same launches again gets
the same keys with NEW image buffers, so the phase's batched job table must go with the evicted entries: kept by key
alone it would send the batched pack launch to the freed buffers.  (Alternating ``infer`` heads on one model -- two
SceneInference objects, say -- evicts and re-records a pruned phase.)  Host only: the launch is replaced by a recorder."""
import ctypes

import torch


class _Weight:   # what PackPlan.image_for reads of an ops.WSrc
    def __init__(self):
        self.t = torch.zeros(4)
        self.device = self.t.device

    def fill(self, dst):
        dst.src = self.t.data_ptr()


def test_evicted_entries_take_their_job_table_with_them(monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    seen = []

    class _Lib:
        @staticmethod
        def unetpp_gemm_pack_weight_images(table, n, max_floats, stream):
            jobs = ctypes.cast(table, ctypes.POINTER(_lib.PackJob))
            seen.append([int(jobs[i].image) for i in range(n)])
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: _Lib)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    plan, w, d = ops.PackPlan(), _Weight(), _lib.GemmDesc()
    d.taps, d.n_in, d.n_out = 9, 1, 1

    def one_pass(phase, sig):
        plan.begin(phase)
        image, ready = plan.image_for(sig, 64, w, d)
        return image, ready

    first, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert not ready and seen == []                               # recorded; packed by the caller this once
    again, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert ready and again is first and seen[-1] == [first.data_ptr()]
    keep = first                                                  # (the old buffer stays allocated: addresses stay distinct)
    for _ in range(20):                                           # another head's passes: fwd/1 goes unused and is evicted
        one_pass("fwd/2", ("fwd/2", "b"))
    assert ("fwd/1", "a") not in plan.entries
    fresh, ready = one_pass("fwd/1", ("fwd/1", "a"))              # recorded again: a new image under the same key
    assert not ready and fresh.data_ptr() != keep.data_ptr()
    n = len(seen)
    _, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert ready and len(seen) == n + 1
    assert seen[-1] == [fresh.data_ptr()], "the batched launch was sent to the evicted entry's buffer"


def _copy_plan(monkeypatch):
    """-> (plan, seen, one_pass): unetpp_copy_jobs is a recorder of the destinations its table names"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    seen = []

    class _Lib:
        @staticmethod
        def unetpp_copy_jobs(table, n, max_elems, stream):
            jobs = ctypes.cast(table, ctypes.POINTER(_lib.CopyJob))
            seen.append([int(jobs[i].dst) for i in range(n)])
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: _Lib)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    plan, src, made = ops.PackPlan(), torch.zeros(8), []

    def one_pass(phase, key, srcsig=0):
        def make():   # one copy of 2 x 4 floats into a new destination
            made.append(torch.zeros(8))
            return made[-1], [src], [(src, 0, 0, 2, 4, 4, 4)]
        plan.begin(phase)
        return plan.copy_for(key, phase, srcsig, make)

    return plan, seen, one_pass


def test_evicted_copies_take_their_job_table_with_them(monkeypatch):
    """the scenario of the image test through copy_for"""
    plan, seen, one_pass = _copy_plan(monkeypatch)
    first, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert not ready and seen == []                               # recorded; filled by the caller this once
    again, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert ready and again is first and seen[-1] == [first.data_ptr()] and plan.copy_launches == 1
    for _ in range(20):                                           # another head's passes: fwd/1 goes unused and is evicted
        one_pass("fwd/2", ("fwd/2", "b"))
    assert ("fwd/1", "a") not in plan.copies and ("fwd/2", "b") in plan.copies
    fresh, ready = one_pass("fwd/1", ("fwd/1", "a"))              # recorded again: a new destination under the same key
    assert not ready and fresh.data_ptr() != first.data_ptr()     # (`first` is still allocated: the addresses are distinct)
    n = len(seen)
    _, ready = one_pass("fwd/1", ("fwd/1", "a"))
    assert ready and len(seen) == n + 1 and plan.launches == 0
    assert seen[-1] == [fresh.data_ptr()], "the batched copy launch was sent to the evicted group's buffer"


def test_pinned_copies_are_kept_and_replaced_tables_retired(monkeypatch):
    plan, seen, one_pass = _copy_plan(monkeypatch)
    first, _ = one_pass("fwd/1", ("fwd/1", "a"))
    one_pass("fwd/1", ("fwd/1", "a"))
    table = plan._copy_tables["fwd/1"]
    plan.pin()
    for _ in range(20):
        one_pass("fwd/2", ("fwd/2", "b"))
    assert ("fwd/1", "a") in plan.copies and plan._copy_tables["fwd/1"] is table and plan._retired == []
    again, ready = one_pass("fwd/1", ("fwd/1", "a"))              # nothing was evicted: the same buffer, the same table
    assert ready and again is first and seen[-1] == [first.data_ptr()] and plan._copy_tables["fwd/1"] is table
    fresh, ready = one_pass("fwd/1", ("fwd/1", "a"), srcsig=1)    # other sources: the group is recorded again
    assert not ready and fresh.data_ptr() != first.data_ptr()
    assert any(t is table for t in plan._retired), "a captured launch may still read the replaced table"
    _, ready = one_pass("fwd/1", ("fwd/1", "a"), srcsig=1)
    assert ready and seen[-1] == [fresh.data_ptr()] and plan._copy_tables["fwd/1"] is not table
    second = plan._copy_tables["fwd/1"]
    plan.copy_for(("fwd/1", "c"), "fwd/1", 0, lambda: (torch.zeros(8), [], []))   # one more group in the phase: other keys
    plan.begin("fwd/1")
    assert plan._copy_tables["fwd/1"] is not second and any(t is second for t in plan._retired)
    plan.unpin()
    assert plan._retired == []
