"""The launch rules of the streaming kernels (BatchNorm apply and pool, pool backward, BatchNorm backward in training and
frozen mode, fp32 and bf16), restated launcher by launcher as commit a6066eb -- the last one whose launchers selected for
themselves -- states them in pointwise.hip and pointwise_bf16.hip.  tests/test_gpu_streaming.py and
tests/test_gpu_bn_frozen.py predict labels, grids and partial rows of real launches from them; tests/test_stream_select.py
holds csrc/stream_select.h against them query by query.  Nothing here reads the header.

A query is a dict: op, bf16, N, H, W, C; the flags scale, shift, act, pooled, idx, dpooled, stats (mean and invstd),
partial, gate for the optional arguments that were given; and the low four address bits per pointer role in_lo (y, d_act),
out_lo (act, dy; d_act of the pool backward), pooled_lo, idx_lo, coef_lo (scale | shift), stat_lo (mean | invstd),
gamma_lo (gamma | dgamma | dbeta), gate_lo -- 0 for a pointer that was not given."""
import torch

OK, EINVAL = 0, -1
AFFINE, POOL_BWD, BN_REDUCE, BN_APPLY, BN_FROZEN = range(5)
K_THREADS = 256
GRID_CAP = 2048 * 8               # grid_for / grid_for8
ROW_CAP = 16384                   # row-structured kernels
REDUCE_CAP = 2048                 # bn_bwd_blocks_for / unetpp_bn_bwd_blocks_bf16
FROZEN_CAP = 2048                 # bn_frozen_blocks_for / unetpp_bn_frozen_bwd_blocks_bf16: workgroups before the grid-stride loop
LIMIT = 0x7fffffff
REFUSED = ("-", 0, 0, 0, 0)
FLAGS = ("scale", "shift", "act", "pooled", "idx", "dpooled", "stats", "partial", "gate")
ROLES = ("in_lo", "out_lo", "pooled_lo", "idx_lo", "coef_lo", "stat_lo", "gamma_lo", "gate_lo")


def lo(*tensors):
    """Low four address bits of a pointer role: OR-ed over its tensors, None counting as not given."""
    bits = 0
    for t in tensors:
        if t is not None:
            bits |= t.data_ptr() & 15
    return bits


def a16(bits):
    return bits & 15 == 0


def al16(t):
    return t is None or t.data_ptr() % 16 == 0


def shifted(t, nbytes=4):
    """The same values in a slice of a longer tensor that starts `nbytes` past a 16-byte boundary."""
    k = nbytes // t.element_size()
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def grid_for(items):   # common.h grid_for
    return max(1, min(GRID_CAP, -(-items // K_THREADS)))


def fin_threads(rows):   # pointwise.hip fin_threads
    return 1024 if rows >= 4096 else 512 if rows >= 1024 else 256


def rows_form_ok(n, h, w, c):   # pointwise.hip rows_form_ok
    return n * h * w * c < 0x7fffffff and (w // 2) * (c // 4) >= 64


def bn_bwd_blocks_for(pixels, c, vec):   # pointwise.hip bn_bwd_blocks_for
    cg = c // 4 if vec else c
    want = max(1, min(REDUCE_CAP, -(-pixels * cg // (K_THREADS * 16))))
    return -(-want // cg) * cg


def bn_bwd_blocks(pixels, c):   # unetpp_bn_bwd_blocks
    return max(bn_bwd_blocks_for(pixels, c, True) if c % 4 == 0 else 0, bn_bwd_blocks_for(pixels, c, False))


def bn_bwd_blocks_bf16(pixels, c):   # unetpp_bn_bwd_blocks_bf16
    return max(1, min(REDUCE_CAP, -(-pixels * (c // 8) // (4 * K_THREADS))))


def frozen_blocks_for(pixels, c, vec):   # pointwise.hip bn_frozen_blocks_for
    cg = c // 4 if vec else c
    want = max(1, min(FROZEN_CAP, -(-pixels * cg // K_THREADS)))
    return -(-want // cg) * cg


def frozen_blocks(pixels, c):   # unetpp_bn_frozen_bwd_blocks
    return max(frozen_blocks_for(pixels, c, True) if c % 4 == 0 else 0, frozen_blocks_for(pixels, c, False))


def frozen_blocks_bf16(pixels, c):   # unetpp_bn_frozen_bwd_blocks_bf16
    return max(1, min(FROZEN_CAP, -(-pixels * (c // 8) // K_THREADS)))


def bn_bwd_pool_ok(n, h, w, c):   # pointwise.hip bn_bwd_pool_ok
    if n < 1 or h < 2 or w < 2 or c < 4 or h & 1 or w & 1 or c & 3:
        return False
    cg = c >> 2
    return cg & (cg - 1) == 0 and cg <= K_THREADS and n * h * w * c < 0x7fffffff


def octets_ok(c):   # pointwise_bf16.hip octets_ok
    cg = c >> 3
    return c >= 8 and c & 7 == 0 and cg & (cg - 1) == 0 and cg <= 256


def partial_rows(bf16, frozen, pixels, c):
    """The four unetpp_*_blocks exports (0 for a shape without a kernel)."""
    if pixels < 1 or c < 1 or (bf16 and not octets_ok(c)):
        return 0
    if bf16:
        return frozen_blocks_bf16(pixels, c) if frozen else bn_bwd_blocks_bf16(pixels, c)
    return frozen_blocks(pixels, c) if frozen else bn_bwd_blocks(pixels, c)


def windows(t):
    """NHWC -> the four candidates of every 2x2 window in scan order (0,0),(0,1),(1,0),(1,1): views [N, H//2, W//2, C]
    (odd H / W: the last row / column is in no window)."""
    h2, w2 = t.shape[1] // 2 * 2, t.shape[2] // 2 * 2
    return [t[:, (q >> 1):h2:2, (q & 1):w2:2, :] for q in range(4)]


def ref_route(d_pooled, idx, shape):
    """float64 NHWC tensor of `shape`: d_pooled at the recorded winner of every window, zero elsewhere."""
    out = torch.zeros(shape, dtype=torch.float64, device=d_pooled.device)
    dp = d_pooled.double()
    for q, v in enumerate(windows(out)):
        v.copy_(torch.where(idx == q, dp, torch.zeros_like(dp)))
    return out


# ------------------------------------------------------------------ one function per launcher: (rc, (label, grid, block,
# rows of the partial buffer, rows the grid writes)); the NULL checks of required pointers are the launcher's own
def _ok(label, grid, buf_rows=0, rows=0):
    return OK, (label, grid, K_THREADS, buf_rows, rows)


def _no():
    return EINVAL, REFUSED


def affine(q):   # unetpp_affine_relu_pool
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if n < 1 or h < 1 or w < 1 or c < 1 or q["scale"] != q["shift"] or not (q["act"] or q["pooled"]):
        return _no()
    vec = c % 4 == 0 and a16(q["in_lo"]) and a16(q["out_lo"]) and a16(q["pooled_lo"])
    if not q["pooled"]:
        return _ok("affine_relu<4>", grid_for(n * h * w * (c // 4))) if vec else _ok("affine_relu<1>", grid_for(n * h * w * c))
    if h < 2 or w < 2:
        return _no()
    win = n * (h // 2) * (w // 2)
    if h & 1 or w & 1:   # apply pass over the whole tensor (when act is wanted), then the window kernel on it
        src = q["out_lo"] if q["act"] else q["in_lo"]
        vec = c % 4 == 0 and a16(src) and a16(q["pooled_lo"])
    elif vec and rows_form_ok(n, h, w, c) and (not q["scale"] or a16(q["coef_lo"])) and q["idx_lo"] & 3 == 0:
        return _ok("affine_relu_pool_rows", min(n * (h // 2), ROW_CAP))
    return _ok("affine_relu_pool<4>", grid_for(win * (c // 4))) if vec else _ok("affine_relu_pool<1>", grid_for(win * c))


def affine_bf16(q):   # unetpp_affine_relu_pool_bf16
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if n < 1 or h < 1 or w < 1 or c < 8 or c & 7 or not a16(q["in_lo"]) or (q["act"] and not a16(q["out_lo"])):
        return _no()
    if q["scale"] != q["shift"] or not (q["act"] or q["pooled"]):
        return _no()
    if not q["pooled"]:
        return _ok("affine_relu_bf16", grid_for(n * h * w * (c >> 3)))
    if h & 1 or w & 1 or not q["idx"] or not a16(q["pooled_lo"]) or q["idx_lo"] & 7:
        return _no()
    items = n * (h // 2) * (w // 2) * (c >> 3)
    return _no() if items >= LIMIT else _ok("affine_relu_pool_bf16", grid_for(items))


def maxpool_bwd(q):   # unetpp_maxpool_bwd
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if n < 1 or h < 2 or w < 2 or c < 1:
        return _no()
    win = n * (h // 2) * (w // 2)
    if (not (h & 1) and not (w & 1) and c % 4 == 0 and rows_form_ok(n, h, w, c) and a16(q["pooled_lo"]) and a16(q["out_lo"])
            and q["idx_lo"] & 3 == 0):
        return _ok("maxpool_bwd_rows", min(n * (h // 2), ROW_CAP))
    return _ok("maxpool_bwd<4>", grid_for(win * (c // 4))) if c % 4 == 0 else _ok("maxpool_bwd<1>", grid_for(win * c))


def maxpool_bwd_bf16(q):   # unetpp_maxpool_bwd_bf16
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if n < 1 or h < 2 or w < 2 or h & 1 or w & 1 or c < 8 or c & 7:
        return _no()
    if not a16(q["pooled_lo"]) or not a16(q["out_lo"]) or (q["gate"] and not a16(q["gate_lo"])) or q["idx_lo"] & 7:
        return _no()
    items = n * h * w * (c >> 3)
    return _no() if items >= LIMIT else _ok("maxpool_bwd_bf16", grid_for(items))


def bn_bwd_reduce(q):   # unetpp_bn_bwd_reduce (pixels = N * H * W)
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if pixels < 1 or c < 1:
        return _no()
    vec = c % 4 == 0 and a16(q["in_lo"])
    blocks = bn_bwd_blocks_for(pixels, c, vec)
    return _ok("bn_bwd_reduce<4>" if vec else "bn_bwd_reduce<1>", blocks, bn_bwd_blocks(pixels, c), blocks)


def bn_bwd_apply(q):   # unetpp_bn_bwd_apply
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if pixels < 1 or c < 1:
        return _no()
    vec = c % 4 == 0 and a16(q["in_lo"]) and a16(q["out_lo"])
    return _ok("bn_bwd_apply<4>", grid_for(pixels * (c // 4))) if vec else _ok("bn_bwd_apply<1>", grid_for(pixels * c))


def bn_bwd_reduce_pool(q):   # unetpp_bn_bwd_reduce_pool
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if not (q["dpooled"] and q["idx"]) or not bn_bwd_pool_ok(n, h, w, c):
        return _no()
    if not (a16(q["in_lo"]) and a16(q["coef_lo"]) and a16(q["stat_lo"]) and a16(q["pooled_lo"])) or q["idx_lo"] & 3:
        return _no()
    buf = bn_bwd_blocks(n * h * w, c)
    return _ok("bn_bwd_reduce_pool", min(n * h, buf), buf, min(n * h, buf))


def bn_bwd_apply_pool(q):   # unetpp_bn_bwd_apply_pool
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if not (q["dpooled"] and q["idx"]) or not bn_bwd_pool_ok(n, h, w, c):
        return _no()
    if (not (a16(q["in_lo"]) and a16(q["out_lo"]) and a16(q["coef_lo"]) and a16(q["stat_lo"]) and a16(q["gamma_lo"])
                and a16(q["pooled_lo"])) or q["idx_lo"] & 3):
        return _no()
    return _ok("bn_bwd_apply_pool", min(n * h, ROW_CAP))


def _bf16_bn_args(q):
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if n < 1 or h < 1 or w < 1 or not octets_ok(c):
        return False
    return q["dpooled"] == q["idx"] and not (q["dpooled"] and (h | w) & 1)


def bn_bwd_reduce_bf16(q):   # unetpp_bn_bwd_reduce_bf16
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if not _bf16_bn_args(q) or pixels * (c >> 3) >= LIMIT:
        return _no()
    blocks = bn_bwd_blocks_bf16(pixels, c)
    return _ok("bn_bwd_reduce_bf16/pool" if q["dpooled"] else "bn_bwd_reduce_bf16", blocks, blocks, blocks)


def bn_bwd_apply_bf16(q):   # unetpp_bn_bwd_apply_bf16
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if not _bf16_bn_args(q) or pixels * (c >> 3) >= LIMIT:
        return _no()
    return _ok("bn_bwd_apply_bf16/pool" if q["dpooled"] else "bn_bwd_apply_bf16", grid_for(pixels * (c >> 3)))


def bn_frozen_bwd(q):   # unetpp_bn_frozen_bwd
    n, h, w, c = q["N"], q["H"], q["W"], q["C"]
    if c < 1 or n < 1 or h < 1 or w < 1 or (q["partial"] and not q["stats"]) or q["dpooled"] != q["idx"]:
        return _no()
    pixels, sums = n * h * w, "/sums" if q["partial"] else ""
    buf = frozen_blocks(pixels, c)
    if q["dpooled"]:
        if not bn_bwd_pool_ok(n, h, w, c):
            return _no()
        if (not (a16(q["in_lo"]) and a16(q["out_lo"]) and a16(q["coef_lo"]) and a16(q["pooled_lo"])) or q["idx_lo"] & 3
                or (q["partial"] and not a16(q["stat_lo"]))):
            return _no()
        grid = min(n * h, buf)
        return _ok("bn_frozen_bwd_pool" + sums, grid, *((buf, grid) if q["partial"] else ()))
    vec = c % 4 == 0 and a16(q["in_lo"]) and a16(q["out_lo"])
    blocks = frozen_blocks_for(pixels, c, vec)
    return _ok(("bn_frozen_bwd<4>" if vec else "bn_frozen_bwd<1>") + sums, blocks, *((buf, blocks) if q["partial"] else ()))


def bn_frozen_bwd_bf16(q):   # unetpp_bn_frozen_bwd_bf16
    pixels, c = q["N"] * q["H"] * q["W"], q["C"]
    if not _bf16_bn_args(q) or (q["partial"] and not q["stats"]):
        return _no()
    if not (a16(q["in_lo"]) and a16(q["out_lo"])) or (q["dpooled"] and not a16(q["pooled_lo"])) or q["idx_lo"] & 7:
        return _no()
    if pixels * (c >> 3) >= LIMIT:
        return _no()
    blocks = frozen_blocks_bf16(pixels, c)
    label = "bn_frozen_bwd_bf16" + ("/pool" if q["dpooled"] else "") + ("/sums" if q["partial"] else "")
    return _ok(label, blocks, *((blocks, blocks) if q["partial"] else ()))


def launcher_of(q):
    """The launcher a query stands for: the fp32 training passes have one entry point with and one without a pool gradient."""
    if q["op"] == AFFINE:
        return affine_bf16 if q["bf16"] else affine
    if q["op"] == POOL_BWD:
        return maxpool_bwd_bf16 if q["bf16"] else maxpool_bwd
    if q["op"] == BN_FROZEN:
        return bn_frozen_bwd_bf16 if q["bf16"] else bn_frozen_bwd
    pool = q["dpooled"] or q["idx"]
    if q["op"] == BN_REDUCE:
        return bn_bwd_reduce_bf16 if q["bf16"] else bn_bwd_reduce_pool if pool else bn_bwd_reduce
    return bn_bwd_apply_bf16 if q["bf16"] else bn_bwd_apply_pool if pool else bn_bwd_apply


# ------------------------------------------------------------------ labels of real launches, from tensors
def expect_affine(y, scale, shift, act, pooled, idx):
    """Label of unetpp_affine_relu_pool[_bf16] from the launcher's conditions."""
    n, h, w, c = y.shape
    q = dict(op=AFFINE, bf16=y.dtype == torch.bfloat16, N=n, H=h, W=w, C=c, scale=scale is not None, shift=shift is not None,
             act=act is not None, pooled=pooled is not None, idx=idx is not None, in_lo=lo(y), out_lo=lo(act),
             pooled_lo=lo(pooled), idx_lo=lo(idx), coef_lo=lo(scale, shift))
    rc, ans = launcher_of(q)(q)
    assert rc == OK, q
    return ans[0]


def expect_maxpool_bwd(d_pooled, idx, d_act, gate=None):
    n, h, w, c = d_act.shape
    q = dict(op=POOL_BWD, bf16=d_act.dtype == torch.bfloat16, N=n, H=h, W=w, C=c, gate=gate is not None, out_lo=lo(d_act),
             pooled_lo=lo(d_pooled), idx_lo=lo(idx), gate_lo=lo(gate))
    rc, ans = launcher_of(q)(q)
    assert rc == OK, q
    return ans[0]
