"""Heat maps <-> key points on the device: the reference's ``Heatmap`` helper.

Mirrors the interface of /root/reference/tools/misc/heatmap.py (class ``Heatmap(HeatmapPattern)``: constructor and its
argument checks :21-54, ``create_heatmap`` :203-230, ``extract_points_`` :148-200, ``transfer_points`` :241-263) that the
reference's validation loop drives on the CPU with numpy + OpenCV for every head output (trainer/trainer.py:213-221).
Here the maps never leave the GPU.

**Parity unpinned.**  The reference file imports OpenCV at module level and OpenCV is absent from the build image, so
no vectors could be generated from it; the kernels are checked against oracle/keypoints_oracle.py (a restatement from
the source text and, for the OpenCV calls of region_segment_ (:100-144), from their published algorithms: the 3x3
chamfer ``cv2.distanceTransform`` in fixed point, cores above a tenth of its maximum, ``cv2.connectedComponents`` of the
cores, ``cv2.watershed`` of the binary mask seeded with them).  ``segmentation="watershed"`` (default) is that region
step: blobs that touch through a thin neck are split, a blob without a core is dropped, the frame of the map (first /
last row and column) belongs to no region, as ``cv2.watershed`` leaves it; ``segmentation="components"`` keeps the round-2
stand-in (a region = an 8-connected component of the mask).  The reference's matcher ``match_distmin`` is unfinished and returns ``[]`` (:56-79): ``transfer_points`` returns
the extracted points in peak order instead of an empty tensor.  ``match_points`` (and ``match_distmin``, the reference's
single-map signature) finishes the matcher on the device: predictions are assigned to the map's labels by the greedy
global minimum of the squared distance (csrc/validate.hip); ``validate.validate_step`` runs it for every head of a batch.

The flood has both levels of the two-valued image: level-0 rounds until nothing moves, one round across the mask's edge
(level 255), level 0 again, until such a round changes nothing -- a hole narrower than 5 px that a region encloses takes
that region's label, and a bright pixel inside it is the region's peak, as in OpenCV.

Known differences of ``"watershed"`` from ``cv2.watershed`` (neither can be pinned without OpenCV; the row stays "parity
unpinned"): (2) the flood runs in synchronous rounds instead of OpenCV's FIFO queues, which moves the line where two
labels meet -- between two touching blobs, in a hole on that line, in the unknown ring beside the frame.  Against the
pixel-by-pixel restatement of the published algorithm (``oracle.keypoints_oracle.watershed_fifo``) on the 200 random
blob-and-hole maps of tests/keypoints_corpus.py: 111 of 42903 region pixels differ (0.26 %), 16 of them sit in two
different regions, at most 9 on one map, and a reported point differs on 3 maps (1.5 %), all three through a ring pixel
beside the frame; the constructed hole cases have identical label maps.  (3) the core threshold float32(0.1 * max)
assumes the float64 product of NumPy < 2 and OpenCV's fixed-point (non-IPP) distance path.  (The numbering is kept:
(1), the missing level-255 phase, is gone.)
"""
from __future__ import annotations

import logging

import torch

from . import _lib, ops


class Heatmap:
    def __init__(self, pattern, w, h, radius=3, match_method="match_distmin", segmentation="watershed"):
        # the argument checks of HeatmapPattern.__init__ (heatmap.py:32-49)
        if not isinstance(pattern, list):
            raise TypeError("'pattern' must be list.")
        if len(pattern) > 4:
            logging.warning("Elements of 'pattern' is suggested to be less than 4.")
        for ele in pattern:
            if not isinstance(ele, list):
                raise TypeError("'pattern' must be list with elements as type 'list'. e.g. [[0,1,3],[2,4],[5]]")
        flat = sum(pattern, [])
        if len(set(flat)) != len(flat):
            raise ValueError("Number in 'pattern' must not repeat.")
        if not isinstance(w, int) or not isinstance(h, int):
            raise TypeError("'w'& 'h' must be int")
        if not isinstance(match_method, str):
            raise TypeError("'match_method' must be str")
        self.pattern, self.w, self.h, self.radius = pattern, w, h, radius
        self.match_method = match_method
        if segmentation not in ("watershed", "components"):
            raise ValueError("'segmentation' must be 'watershed' or 'components'")
        self.segmentation = segmentation

    @staticmethod
    def _cuda(t):
        t = torch.as_tensor(t, dtype=torch.float32)
        if not t.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("Heatmap runs on the GPU: this path has no CPU fallback")
            t = t.cuda()
        return t.contiguous()

    def create_heatmap(self, targets) -> torch.Tensor:
        """targets [N, C, 2] as (x, y) -> CUDA float32 [N, len(pattern), H, W]  (heatmap.py:203-230)"""
        return ops.heatmap_pattern(self._cuda(targets), self.pattern, self.h, self.w, float(self.radius))

    def extract_points_(self, pred, num, threshold=0.5):
        """[H, W] heat map -> list of up to `num` [x, y], brightest region first (heatmap.py:148-200)"""
        pred = self._cuda(pred)
        if pred.dim() != 2:
            raise AssertionError("Heatmap assertion failed. It should be [H, W]")
        points, counts = ops.keypoints_extract(pred.unsqueeze(0), int(num), float(threshold), segmentation=self.segmentation)
        n = min(int(counts[0]), int(num))
        # origin size == map size here (the reference rescales by origin/self sizes that are the same numbers, :171-172)
        return [[int(x), int(y)] for x, y in points[0, :n].cpu().tolist()]

    def transfer_points(self, preds, targets=None, threshold=0.5):
        """preds [N, C, H, W] -> (points [N, C, max_num, 2] CUDA float32 as (x, y), -1 padded; counts [N, C] int32 =
        points found per map).  `targets` is accepted for signature compatibility (heatmap.py:241): the reference
        only uses it in its unfinished matcher.  The points stay in peak order; ``match_points(points, counts, targets)``
        assigns them to the labels."""
        preds = self._cuda(preds)
        if preds.dim() != 4:
            raise AssertionError("preds shape should be [N, C, H, W]")
        if preds.shape[1] != len(self.pattern):
            raise AssertionError("2nd dimension of preds must equal the number of maps of the pattern")
        if targets is not None:
            t = torch.as_tensor(targets)
            if t.dim() != 3 or t.shape[2] != 2 or t.shape[0] != preds.shape[0]:
                raise AssertionError("targets shape should be [N, C, 2] with the batch size of preds")
        n, c, h, w = preds.shape
        nums = [len(hmap) for hmap in self.pattern]
        points, counts = ops.keypoints_extract(preds.view(n * c, h, w), max(nums), float(threshold),
                                               segmentation=self.segmentation)
        points, counts = points.view(n, c, max(nums), 2), counts.view(n, c)
        limit = torch.tensor(nums, dtype=torch.int32, device=points.device).view(1, c)
        found = torch.minimum(counts, limit)
        slot = torch.arange(max(nums), device=points.device).view(1, 1, -1)
        points = torch.where((slot < found.unsqueeze(-1)).unsqueeze(-1), points, torch.full_like(points, -1.0))
        return points, found

    def match_points(self, points, found, targets):
        """points [N, C, K, 2] and found [N, C] as ``transfer_points`` returns them, targets [N, S, 2] as (x, y) ->
        (matched [N, S, 2] CUDA float32: the prediction assigned to label s, (-1, -1) where none; mask [N, S] bool).
        The rule the reference's ``match_distmin`` left open (heatmap.py:57-79): per map, min(labels, predictions) times
        the pair of an unassigned label of ``pattern[c]`` and an unused prediction with the smallest (squared distance,
        position of the label in the map's list, prediction index) is assigned (csrc/validate.hip).  Labels that no map
        of the pattern holds are never matched."""
        points, targets = self._cuda(points), self._cuda(targets)
        found = torch.as_tensor(found).to(device=points.device, dtype=torch.int32).contiguous()
        if points.dim() != 4 or points.shape[3] != 2 or points.shape[1] != len(self.pattern):
            raise ValueError("points must be [N, len(pattern), K, 2]")
        if tuple(found.shape) != tuple(points.shape[:2]):
            raise ValueError("found must be [N, len(pattern)]")
        if targets.dim() != 3 or targets.shape[2] != 2 or targets.shape[0] != points.shape[0]:
            raise ValueError("targets must be [N, S, 2] with the batch size of points")
        n, c, k = points.shape[:3]
        matched, mask, _, _ = ops.match_points(points.reshape(n * c, k, 2), found.view(-1), targets, self.pattern)
        return matched[0], mask[0]

    def match_distmin(self, predpoints, targets, index_list):
        """The reference's single-map matcher (heatmap.py:57-79): predicted points of one map (list of [x, y]), all key
        points of the image (targets [S, 2]) and the map's label indices -> a list of [x, y] in ``index_list`` order, the
        prediction matched to each label or [-1, -1].  Same rule and same kernel as ``match_points``."""
        pred = torch.as_tensor(predpoints, dtype=torch.float32).reshape(-1, 2)
        if pred.shape[0] > _lib.MATCH_MAX:
            raise ValueError("at most %d predicted points per map" % _lib.MATCH_MAX)
        labels = torch.as_tensor(targets, dtype=torch.float32)
        if labels.dim() != 2 or labels.shape[1] != 2:
            raise ValueError("targets must be [S, 2]")
        index_list = [int(i) for i in index_list]
        ops.check_match_pattern([index_list], labels.shape[0])
        padded = torch.full((1, max(1, pred.shape[0]), 2), -1.0)
        padded[0, :pred.shape[0]] = pred
        points = self._cuda(padded)
        found = torch.full((1,), pred.shape[0], dtype=torch.int32, device=points.device)
        matched, _, _, _ = ops.match_points(points, found, self._cuda(labels).unsqueeze(0), [index_list])
        return matched[0, 0, index_list].tolist()
