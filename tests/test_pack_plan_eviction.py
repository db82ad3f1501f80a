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
