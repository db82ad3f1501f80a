"""Scene inference: the eval forward of UNet_Nested over frames far larger than the geometry the kernels are tuned for,
exact rather than blended, with dihedral test-time augmentation folded into the stitch (csrc/scene.hip).

    scene = SceneInference(model.eval(), head=3, tile=512, tta="dihedral")
    maps = scene(frames)                      # uint8 [S, H, W, C] or float32 [S, C, H, W] on the GPU -> [S, n_classes, H, W]
    points, counts = scene.points(maps, heatmap)
    dets = scene.detect(frames, PeakDetector())   # any number of objects per map (detect.py)
    cascade = CascadeSceneInference(model.eval(), head=3, screen_head=1, threshold=0.1, tta="dihedral")
    maps = cascade(frames)                    # head 1 everywhere, head 3 only on the tiles where head 1 fires

The frame is cut into overlapping tiles of one fixed shape; chunks of tiles run through ``model.infer`` (or one captured
``GraphedForward``) and ``unetpp_scene_stitch`` puts each tile's OWNED interior back.  Why the result equals the
whole-frame forward: in eval mode with the transposed-convolution up path head J has a finite receptive
field of radius r_J = 7 * 2^J - 5 pixels; a pixel at least that far from every cut edge of its tile sees exactly the
inputs it would see in the frame, and a tile edge that IS a frame edge sees the same zero padding.  Tile origins are
multiples of A = 2^(depth-1), so pooling windows and transposed-convolution phases line up with the frame's.

The reference has no counterpart: its validation loop feeds whole 256x256 images (trainer/trainer.py:141-180).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Tuple

import torch

from . import _lib, engine, ops
from .loader import _per_channel, affine_params
from .serving import GraphedForward

__all__ = ["required_halo", "plan_tiles", "SceneInference", "TTA_VARIANTS", "CascadeSceneInference", "CascadeAudit",
           "screen_rows", "cascade_chunks"]

_FX, _FY, _T = _lib.SCENE_FLIP_X, _lib.SCENE_FLIP_Y, _lib.SCENE_TRANSPOSE
# variant codes (include/unetpp_hip.h): the variant is flip_y(flip_x(transpose(tile))), each step only if its bit is set
TTA_VARIANTS = {None: (0,), "flips": (0, _FX, _FY, _FX | _FY), "dihedral": tuple(range(8))}
_MAX_SIDE = 1 << 24   # pixel indices are exact in fp32 below this (the warp's parameter rows are fp32)


def required_halo(depth: int, head: int) -> int:
    """The least halo at which a tiled forward of head `head` is exact: the head's receptive-field radius
    r_J = 7 * 2^J - 5 (9, 23, 51, 107 for heads 1 to 4; measured on the float64 oracle as the support of the input
    gradient of one head pixel, whatever the depth, the widths or the BatchNorm setting), rounded up to a multiple of
    A = 2^(depth-1), the divisibility the engine demands of H and W."""
    head = engine.check_head(depth, head)
    a = 1 << (depth - 1)
    r = 7 * (1 << head) - 5
    return -(-r // a) * a


def _plan_axis(L: int, tile: int, halo: int) -> List[Tuple[int, int, int]]:
    T = min(tile, L)
    if T == L:
        return [(0, 0, L)]
    s = T - 2 * halo
    if s <= 0:
        raise ValueError("tile %d leaves no interior beside a halo of %d: tile must exceed 2 * halo" % (tile, halo))
    out, k, own_lo = [], 0, 0
    while True:
        o = min(k * s, L - T)
        last = o == L - T
        own_hi = L if last else o + T - halo
        out.append((o, own_lo, own_hi))
        if last:
            return out
        own_lo, k = own_hi, k + 1


def plan_tiles(H: int, W: int, tile: int, halo: int, align: int):
    """(rows, cols): per axis, a list of (origin, own_lo, own_hi) in frame coordinates.  Along an axis of length L the
    tile length is T = min(tile, L); T == L is one tile that owns [0, L).  Otherwise tile k starts at
    min(k * (T - 2 halo), L - T) and owns from where the previous tile's ownership ended (0 for the first) up to
    origin + T - halo, the tile that reaches L - T being the last and owning up to L.  So origins are multiples of
    `align`, the owned intervals partition [0, L), and an owned pixel is at least `halo` from every tile edge that is not
    a frame edge.  H, W, tile and halo must be positive multiples of `align` (halo may be 0)."""
    for name, v in (("H", H), ("W", W), ("tile", tile), ("halo", halo), ("align", align)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
    if align < 1 or H < 1 or W < 1 or tile < 1 or halo < 0:
        raise ValueError("H, W, tile and align must be positive and halo non-negative")
    for name, v in (("H", H), ("W", W), ("tile", tile), ("halo", halo)):
        if v % align:
            raise ValueError("%s = %d is not a multiple of %d" % (name, v, align))
    return _plan_axis(H, tile, halo), _plan_axis(W, tile, halo)


def _variant_forward(code: int, oy: int, ox: int, th: int, tw: int):
    """Forward map (frame pixel -> variant pixel) of the variant `code` of the tile at (oy, ox), as the [2, 3] rows of
    affine_params: whole numbers throughout, so the warp copies pixels bit for bit."""
    sx, cx = (-1, tw - 1) if code & _FX else (1, 0)
    sy, cy = (-1, th - 1) if code & _FY else (1, 0)
    if code & _T:   # variant (row, column) = (x - ox, y - oy), then the flips
        return [[0, sx, cx - sx * oy], [sy, 0, cy - sy * ox]]
    return [[sx, 0, cx - sx * ox], [0, sy, cy - sy * oy]]


class _Chunk:
    __slots__ = ("n", "index", "params", "rects", "rects_dev")


_PAD_TILE = (-1, 0, 0, 0, 0, 0, 0)   # a padding row of a tile table


class SceneInference:
    """scene(frames) -> float32 [S, n_classes, H, W] on the device: head `head` of ``model`` (``None`` = the last; with
    ``ensemble`` the mean of heads 1 .. head) over whole frames, computed tile by tile and equal to what the whole-frame
    forward computes wherever the same kernels are selected (bit for bit equal to per-tile ``model.infer`` outputs placed
    by ownership).

    tile: side of the square tile (a frame side below it becomes the tile's side).  halo: pixels of context around the
    owned interior, default and minimum ``required_halo(depth, head)``.  tta: ``None``, ``"flips"`` (identity, h, v, hv)
    or ``"dihedral"`` (all eight; square tiles only) -- the variants' maps are averaged at the inverse-transformed
    position inside the stitch launch, ``(((v_0 + v_1) + ...) + v_{K-1}) / K``.  chunk: tiles per forward (``chunk * K``
    samples).  mul / add: the DeviceLoader's normalisation, ``pixel * mul[c] + add[c]``, for uint8 and float32 frames
    alike.  graphed: one ``GraphedForward`` captured for the chunk shape serves frames of any size; the last chunk is
    padded with the loader's all-fill samples, which the stitch skips.

    Per chunk: one warp launch (gather, flips and turns, normalisation), the forward, one stitch launch; at most one
    chunk of tile maps is alive.  Tile tables are built once per (S, H, W) and cached."""

    def __init__(self, model, head=None, ensemble: bool = False, tile: int = 512, halo=None, tta=None, chunk: int = 8,
                 mul=1.0 / 255.0, add=0.0, graphed: bool = False):
        depth = getattr(model, "depth", None)
        if depth is None or not hasattr(model, "infer"):
            raise TypeError("SceneInference drives UNet_Nested.infer")
        self.head = engine.check_head(depth, head)
        if model.training:
            raise RuntimeError("SceneInference runs the eval forward: call model.eval() first")
        if not model.is_deconv:
            raise ValueError(
                "no halo makes a tile exact with the bilinear up path (is_deconv=False): UpsamplingBilinear2d is "
                "align_corners=True, so every output pixel's source position depends on the size of the whole frame")
        self.align = 1 << (depth - 1)
        need = required_halo(depth, self.head)
        halo = need if halo is None else halo
        for name, v in (("tile", tile), ("halo", halo), ("chunk", chunk)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError("%s must be a positive int, got %r" % (name, v))
        if tile % self.align or halo % self.align:
            raise ValueError("tile and halo must be multiples of %d for a depth-%d network, got %d and %d"
                             % (self.align, depth, tile, halo))
        if halo < need:
            raise ValueError("head %d of a depth-%d network needs a halo of %d (receptive-field radius %d), got %d"
                             % (self.head, depth, need, 7 * (1 << self.head) - 5, halo))
        if tile <= 2 * halo:
            raise ValueError("tile %d leaves no interior beside a halo of %d: tile must exceed 2 * halo" % (tile, halo))
        if tta not in TTA_VARIANTS:
            raise ValueError("tta is None, 'flips' or 'dihedral', got %r" % (tta,))
        self.model, self.ensemble, self.tile, self.halo, self.chunk = model, bool(ensemble), tile, halo, chunk
        self.tta, self.variants, self.graphed = tta, TTA_VARIANTS[tta], bool(graphed)
        self.mul, self.add = mul, add
        self._plans, self._graphs, self._norm = {}, {}, {}

    # ---- host side ---------------------------------------------------------------------------------
    def tile_shape(self, H: int, W: int) -> Tuple[int, int]:
        return min(self.tile, H), min(self.tile, W)

    def efficiency(self, H: int, W: int) -> float:
        """Owned pixels over computed pixels of one frame (per variant): (400 / 512)^2 = 0.61 for a large frame at tile
        512 and halo 56."""
        rows, cols = plan_tiles(H, W, self.tile, self.halo, self.align)
        th, tw = self.tile_shape(H, W)
        return float(H * W) / float(len(rows) * len(cols) * th * tw)

    def _check_size(self, H: int, W: int) -> None:
        if H >= _MAX_SIDE or W >= _MAX_SIDE:
            raise ValueError("frame sides must be below 2^24 (pixel indices are carried in fp32), got %dx%d" % (H, W))
        if H % self.align or W % self.align:
            raise ValueError("H and W must be divisible by %d, got %dx%d" % (self.align, H, W))
        if self.tta == "dihedral" and (H < self.tile or W < self.tile):
            raise ValueError("tta='dihedral' needs square tiles: both frame sides must reach tile = %d, got %dx%d"
                             % (self.tile, H, W))

    def _tiles(self, S: int, H: int, W: int):
        """every tile of S frames in plan order: rows of (frame, oy, ox, y_lo, y_hi, x_lo, x_hi)"""
        rows, cols = plan_tiles(H, W, self.tile, self.halo, self.align)
        return [(s, oy, ox, y0, y1, x0, x1) for s in range(S) for (oy, y0, y1) in rows for (ox, x0, x1) in cols]

    def _chunk(self, part, th: int, tw: int, device) -> _Chunk:
        """the tables of one forward over the tiles `part` (a row with frame < 0 is an all-fill sample the stitch skips)"""
        identity = _variant_forward(0, 0, 0, th, tw)
        c = _Chunk()
        c.n = len(part)
        c.index = torch.tensor([t[0] for t in part for _ in self.variants], dtype=torch.int64).to(device)
        fwd = [_variant_forward(code, t[1], t[2], th, tw) if t[0] >= 0 else identity
               for t in part for code in self.variants]
        c.params = affine_params(fwd).to(device)
        c.rects = ops.scene_rects(part)
        c.rects_dev = c.rects.to(device)
        return c

    def _plan(self, S: int, H: int, W: int, device) -> List[_Chunk]:
        key = (S, H, W, str(device))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        th, tw = self.tile_shape(H, W)
        tiles = self._tiles(S, H, W)
        plan = []
        for i in range(0, len(tiles), self.chunk):
            part = tiles[i:i + self.chunk]
            if self.graphed:   # the captured shape: pad with all-fill samples that the stitch skips
                part = part + [_PAD_TILE] * (self.chunk - len(part))
            plan.append(self._chunk(part, th, tw, device))
        self._plans[key] = plan
        return plan

    # ---- device side -------------------------------------------------------------------------------
    def _prepare(self, frames: torch.Tensor):
        """checks of a call -> (contiguous frames, S, H, W)"""
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise RuntimeError("frames must live on the GPU: this path has no CPU fallback")
        if frames.dtype not in (torch.uint8, torch.float32):
            raise TypeError("frames must be uint8 [S, H, W, C] or float32 [S, C, H, W], got %s" % frames.dtype)
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4:
            raise ValueError("frames must be uint8 [S, H, W, C] or float32 [S, C, H, W] (or one frame without S)")
        u8 = frames.dtype == torch.uint8
        S = int(frames.shape[0])
        H, W, cin = (int(v) for v in (frames.shape[1:] if u8 else (frames.shape[2], frames.shape[3], frames.shape[1])))
        if cin != self.model.in_channels:
            raise ValueError("expected %d input channels, got %d" % (self.model.in_channels, cin))
        if self.model.training:
            raise RuntimeError("SceneInference runs the eval forward: call model.eval() first")
        self._check_size(H, W)
        return frames.contiguous(), S, H, W

    def _run(self, frames: torch.Tensor, chunks, out: torch.Tensor) -> torch.Tensor:
        """warp, forward and stitch of every chunk in `chunks` (each of self.chunk tiles when graphed) into out
        [S, n_classes, H, W]; pixels no tile of the chunks owns are left as they are"""
        model, dev = self.model, frames.device
        H, W = int(out.shape[2]), int(out.shape[3])
        cin = model.in_channels
        norm = self._norm.get(str(dev))
        if norm is None:
            norm = self._norm[str(dev)] = (_per_channel(self.mul, cin, dev), _per_channel(self.add, cin, dev))
        th, tw = self.tile_shape(H, W)
        K = len(self.variants)
        graph = self._graph(cin, th, tw, dev) if self.graphed and chunks else None
        for c in chunks:
            if graph is not None:
                x = ops.warp_batch(frames, c.index, c.params, (th, tw), norm[0], norm[1], 0.0, out=graph.static_input)
                maps = graph(x)
            else:
                x = ops.warp_batch(frames, c.index, c.params, (th, tw), norm[0], norm[1], 0.0)
                maps = model.infer(x, self.head, self.ensemble)
            ops.scene_stitch(maps.view(c.n, K, model.n_classes, th, tw), c.rects, c.rects_dev, self.variants, out)
        return out

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        frames, S, H, W = self._prepare(frames)
        out = torch.empty(S, self.model.n_classes, H, W, dtype=torch.float32, device=frames.device)
        return self._run(frames, self._plan(S, H, W, frames.device), out)

    def uncertainty(self, frames: torch.Tensor, samples: int = 16, seed: int = 0) -> engine.McMaps:
        """Monte-Carlo dropout over whole frames -> ``McMaps(mean, var)``, each float32 [S, n_classes, H, W]: where the
        head's response depends on which features are present -- which unlabelled region to label next, where a screen
        threshold sits on unstable responses.

        The plan, the gather and the ownership of ``__call__``, eager only (``graphed`` is not used here): chunk i of the
        plan is ONE ``model.infer_mc(tiles, head, samples, seed=chunk_seed(seed, i))`` over its batch of tiles, and the
        tiles' mean maps and variance maps are each put back by the stitch launch as a copy of the owned pixels.  So a
        pixel's statistics are those of ``samples`` draws of the head on the tile that owns it; tiles draw independent
        masks (the keep flags are keyed by the pixel's index in the chunk's batch), and a call is reproducible from
        ``seed``.  Not available with test-time augmentation or the ensemble mean: see the message."""
        if self.tta is not None or self.ensemble:
            raise ValueError(
                "uncertainty() has no form for tta=%r, ensemble=%r: the stitch would average the variants' variance maps, "
                "and a mean of per-variant variances is not the variance of the averaged map (the variants' draws are "
                "independent and their maps are averaged before anything is thresholded); build the scene with tta=None "
                "and ensemble=False" % (self.tta, self.ensemble))
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError("seed must be an int, got %r" % (seed,))
        frames, S, H, W = self._prepare(frames)
        model, dev = self.model, frames.device
        cin = model.in_channels
        norm = self._norm.get(str(dev))
        if norm is None:
            norm = self._norm[str(dev)] = (_per_channel(self.mul, cin, dev), _per_channel(self.add, cin, dev))
        th, tw = self.tile_shape(H, W)
        mean = torch.empty(S, model.n_classes, H, W, dtype=torch.float32, device=dev)
        var = torch.empty_like(mean)
        for i, c in enumerate(self._plan(S, H, W, dev)):   # (a graphed scene's padding samples run too; the stitch skips them)
            x = ops.warp_batch(frames, c.index, c.params, (th, tw), norm[0], norm[1], 0.0)
            maps = model.infer_mc(x, self.head, samples, seed=self.chunk_seed(seed, i))
            for tiles, out in ((maps.mean, mean), (maps.var, var)):
                ops.scene_stitch(tiles.view(c.n, 1, model.n_classes, th, tw), c.rects, c.rects_dev, (0,), out)
        return engine.McMaps(mean, var)

    @staticmethod
    def chunk_seed(seed: int, chunk_index: int) -> int:
        """The ``infer_mc`` seed of chunk `chunk_index` (0-based, plan order) of ``uncertainty(frames, samples, seed)``."""
        return (seed + 0xA0761D6478BD642F * (chunk_index + 1)) & 0xFFFFFFFFFFFFFFFF

    def _graph(self, cin: int, th: int, tw: int, dev) -> GraphedForward:
        key = (cin, th, tw, str(dev))
        g = self._graphs.get(key)
        if g is None:
            example = torch.zeros(self.chunk * len(self.variants), cin, th, tw, dtype=torch.float32, device=dev)
            g = self._graphs[key] = GraphedForward(self.model, example, head=self.head, ensemble=self.ensemble)
        return g

    def points(self, maps: torch.Tensor, heatmap, threshold: float = 0.5):
        """``heatmap.transfer_points`` on the stitched maps.  The extraction works per map and its core threshold is a
        per-map maximum (cores are what lies above a tenth of the map's largest distance value), so it must see the whole
        frame: run on tiles it would judge each tile by its own maximum and find other points.  This is the reference's
        fixed-count extraction (at most ``len(pattern[c])`` points per map); ``detect()`` is the one for scenes."""
        return heatmap.transfer_points(maps, None, threshold)

    def detect(self, frames: torch.Tensor, detector):
        """``detector(self(frames))``: the frames' maps through a ``detect.PeakDetector`` -> ``Detections``."""
        return detector(self(frames))


# ---- cascaded scene inference -----------------------------------------------------------
def screen_rows(tiles, th: int, tw: int, margin: int):
    """The screened rectangle R_t of every deep tile: its owned rectangle O_t grown by `margin` pixels on all four sides,
    then clipped to the tile's own extent [oy, oy + th) x [ox, ox + tw).  Rows in and out are (frame, oy, ox, y_lo, y_hi,
    x_lo, x_hi); margin = 0 returns the owned rectangles, which partition the frame."""
    return [(s, oy, ox, max(y0 - margin, oy), min(y1 + margin, oy + th), max(x0 - margin, ox), min(x1 + margin, ox + tw))
            for (s, oy, ox, y0, y1, x0, x1) in tiles]


def cascade_chunks(active, chunk: int, graphed: bool = False):
    """The deep forwards of one call: the active tile ids, in plan order, cut into lists of at most `chunk`; with
    `graphed` the last list is filled up to `chunk` with -1 (an all-fill sample that the stitch skips), the captured
    shape.  No active tile, no forward: []."""
    ids = [int(i) for i in active]
    out = [ids[i:i + chunk] for i in range(0, len(ids), chunk)]
    if graphed and out:
        out[-1] = out[-1] + [-1] * (chunk - len(out[-1]))
    return out


class CascadeAudit(NamedTuple):
    """What ``CascadeSceneInference.audit`` found at `level`: tiles whose deep score reaches it that the screen left
    inactive, active tiles whose deep score stays below it, and max |cascade - deep| over the frames."""
    missed: int
    wasted: int
    max_abs_diff: float
    n_active: int
    n_tiles: int
    level: float


class _CascadePlan:
    __slots__ = ("n", "tiles", "screen", "screen_dev", "owned", "owned_dev")


class CascadeSceneInference:
    """cascade(frames) -> float32 [S, n_classes, H, W] on the device: the shallow head `screen_head` everywhere, the deep
    head `head` -- with its test-time augmentation and, with ``ensemble``, as the mean of heads 1 .. head -- only on the
    tiles where the shallow head fires.

    The rule.  The deep plan is the one ``SceneInference(model, head, tile=tile, halo=halo, tta=tta, chunk=chunk)``
    builds: tile t of frame s has an origin, a shape and an owned rectangle O_t.  Its screened rectangle R_t is O_t grown
    by ``margin`` pixels on all four sides (default: the deep halo; 0 screens exactly the owned pixels), clipped to the
    tile's extent.  M1 is the whole-frame map of the shallow head, ``SceneInference(model, head=screen_head,
    tile=screen_tile, chunk=screen_chunk)(frames)`` with that head's own, smaller halo.  Over all classes and all pixels
    of R_t:  active_t = any(!(M1 < threshold)) -- a value equal to the threshold activates, and so does a NaN -- and
    score_t = fmax of the values (-inf when all are NaN).  The result starts as M1 (the same buffer, no copy), and every
    active tile's owned rectangle is overwritten with the deep head's value through the same stitch launch:
    ``out == where(A, D, M1)`` bit for bit, D the plain deep ``SceneInference``'s map and A the flag of the tile that owns
    the pixel -- wherever the deep forward selects the same kernels for the cascade's chunks as for the plain scene's.

    Per call: the screen stage, ONE ``unetpp_scene_screen`` launch over all deep tiles of all frames, one copy of the
    ``active`` flags to the host -- THE ONLY DEVICE-TO-HOST COPY OF A CALL: how many deep forwards follow depends on the
    data, so the host has to know -- and the deep stage over the active tiles in plan order, ``chunk`` tiles per forward.
    With no active tile the deep model never runs.  ``graphed`` captures one graph per stage (two live captures on one
    model coexist: each pins the weight-image plan it was captured with); the deep stage's last chunk is padded with
    all-fill samples as in ``SceneInference``.

    The constructor refuses ``screen_head >= head``, a threshold that is not finite, a negative margin, and whatever
    ``SceneInference`` refuses for either stage.  ``threshold`` is a plain attribute: set it between calls (``audit``
    helps to choose it); +inf and -inf then mean "no tile" and "every tile", NaN is refused at the call.

    After a call: ``last_active`` (host bool [n_tiles], plan order), ``last_scores`` (device float32 [n_tiles]),
    ``last_fraction`` (active tiles over tiles) and ``last_forwards`` (deep forwards run)."""

    def __init__(self, model, head=None, screen_head: int = 1, threshold: float = 0.1, ensemble: bool = False,
                 tile: int = 512, screen_tile=None, halo=None, margin=None, tta=None, chunk: int = 8, screen_chunk=None,
                 mul=1.0 / 255.0, add=0.0, graphed: bool = False):
        self.deep = SceneInference(model, head=head, ensemble=ensemble, tile=tile, halo=halo, tta=tta, chunk=chunk,
                                   mul=mul, add=add, graphed=graphed)
        screen_head = engine.check_head(model.depth, screen_head)
        if screen_head >= self.deep.head:
            raise ValueError("the screen head must be shallower than the deep head, got screen_head = %d, head = %d"
                             % (screen_head, self.deep.head))
        self.screen = SceneInference(model, head=screen_head, tile=tile if screen_tile is None else screen_tile,
                                     chunk=chunk if screen_chunk is None else screen_chunk, mul=mul, add=add,
                                     graphed=graphed)
        threshold = float(threshold)
        if not math.isfinite(threshold):
            raise ValueError("threshold must be finite, got %r" % threshold)
        margin = self.deep.halo if margin is None else margin
        if isinstance(margin, bool) or not isinstance(margin, int) or margin < 0:
            raise ValueError("margin must be an int >= 0, got %r" % (margin,))
        self.model, self.threshold, self.margin = model, threshold, margin
        self.head, self.screen_head, self.chunk, self.graphed = self.deep.head, screen_head, chunk, bool(graphed)
        self._plans = {}
        self.last_active = self.last_scores = self._active_dev = None
        self.last_fraction, self.last_forwards = 0.0, 0

    def _plan(self, S: int, H: int, W: int, device) -> _CascadePlan:
        key = (S, H, W, str(device))
        p = self._plans.get(key)
        if p is None:
            deep = self.deep
            th, tw = deep.tile_shape(H, W)
            tiles = deep._tiles(S, H, W)
            p = self._plans[key] = _CascadePlan()
            p.n = len(tiles)
            p.screen = ops.scene_rects(screen_rows(tiles, th, tw, self.margin))
            p.screen_dev = p.screen.to(device)
            p.owned = ops.scene_rects(tiles)
            p.owned_dev = p.owned.to(device)
            p.tiles = deep._chunk(tiles + [_PAD_TILE], th, tw, device)   # row n: the padding sample
        return p

    def _deep_chunks(self, p: _CascadePlan, active, device) -> List[_Chunk]:
        """the tables of the call's deep forwards, gathered on the device from the plan's per-tile tables"""
        groups = cascade_chunks(active, self.chunk, self.graphed)
        if not groups:
            return []
        K = len(self.deep.variants)
        sel = torch.tensor([p.n if i < 0 else i for g in groups for i in g], dtype=torch.int64)
        sel_dev = sel.to(device)
        index = p.tiles.index.view(p.n + 1, K).index_select(0, sel_dev)
        params = p.tiles.params.view(p.n + 1, K, -1).index_select(0, sel_dev)
        rects = p.tiles.rects.index_select(0, sel)
        rects_dev = p.tiles.rects_dev.index_select(0, sel_dev)
        chunks, at = [], 0
        for g in groups:
            c = _Chunk()
            c.n = len(g)
            c.index = index[at:at + c.n].reshape(-1)
            c.params = params[at:at + c.n].reshape(c.n * K, -1)
            c.rects = rects[at:at + c.n].contiguous()
            c.rects_dev = rects_dev[at:at + c.n]
            chunks.append(c)
            at += c.n
        return chunks

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        """The cascade's map of the frames.  Exactly one device-to-host copy happens in a call: the ``active`` flags."""
        threshold = float(self.threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
        frames, S, H, W = self.deep._prepare(frames)
        dev = frames.device
        out = self.screen(frames)                                                   # M1
        p = self._plan(S, H, W, dev)
        active, scores = ops.scene_screen(out, p.screen, p.screen_dev, threshold)
        host = active.cpu() != 0                                                    # the one read-back
        chunks = self._deep_chunks(p, torch.nonzero(host).flatten().tolist(), dev)
        self.deep._run(frames, chunks, out)
        self.last_active, self.last_scores, self._active_dev = host, scores, active
        self.last_fraction = float(int(host.sum())) / p.n
        self.last_forwards = len(chunks)
        return out

    def detect(self, frames: torch.Tensor, detector):
        """``detector(self(frames))`` -> ``Detections``.  Below the screen threshold the cascade is blind by design (an
        inactive tile shows the shallow head's map, all of it below the threshold on its owned pixels), so a detector
        whose threshold lies below the screen's is refused.  What holds at or above it: no detection can come from the
        owned pixels of an inactive tile."""
        if float(detector.threshold) < float(self.threshold):
            raise ValueError("the detector's threshold %g lies below the screen threshold %g: the cascade is blind there"
                             % (detector.threshold, self.threshold))
        return detector(self(frames))

    def audit(self, frames: torch.Tensor, level=None) -> CascadeAudit:
        """The tool for choosing ``threshold``: runs the cascade AND the plain deep scene on the frames, screens the deep
        map D with margin 0 (one more ``unetpp_scene_screen`` launch: deep_score_t = fmax of D over the tile's owned
        pixels) and counts, on the device, the tiles with deep_score_t >= level (default: the threshold) that the screen
        left inactive (missed) and the active tiles whose deep score stays below level (wasted); with max |out - D| these
        few numbers are read back at the end."""
        level = float(self.threshold if level is None else level)
        if level != level:
            raise ValueError("level must not be NaN")
        out = self(frames)
        deep = self.deep(frames)
        p = self._plan(int(out.shape[0]), int(out.shape[2]), int(out.shape[3]), out.device)
        _, deep_score = ops.scene_screen(deep, p.owned, p.owned_dev, level)
        on = self._active_dev != 0
        missed = ((deep_score >= level) & ~on).sum()
        wasted = ((deep_score < level) & on).sum()
        diff = (out - deep).abs().max()
        counts = torch.stack([missed, wasted, on.sum()]).tolist()
        return CascadeAudit(int(counts[0]), int(counts[1]), float(diff), int(counts[2]), p.n, level)
