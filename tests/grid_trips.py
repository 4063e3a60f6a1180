"""Case table for the capped-grid launchers of iseg_amd/csrc: one entry per launcher whose kernel walks its work with a
`gridDim`-strided loop, at a shape that drives the loop through at least TWO FULL TRIPS PLUS A RAGGED THIRD.

Plain Python (no torch): test_grid_trips_host.py checks the arithmetic on any machine, test_grid_trips_gpu.py runs every entry against a
float64 reference on the GPU.

An entry mirrors its launcher: `launcher(dtype, **shape)` returns one `Trip` per kernel the entry point launches,
    Trip(grid, per_trip, items, quantum, tail)
      grid      workgroups the launcher asks for at this shape
      per_trip  work items the whole grid consumes in one pass of the loop (the stride expression of the kernel, in items)
      items     work items of the loop
      quantum   items one workgroup consumes per pass (the ragged trip must not end on a workgroup boundary)
      tail      elements the kernel's scalar tail loop handles after its 16-byte body (None: the kernel has no such loop)
and the rule is   items > 2 * per_trip,  items % per_trip != 0,  items % per_trip % quantum != 0 (quantum > 1),  tail != 0.
`first_of_last_trip(trip)` is the first item of the ragged trip; the GPU tests assert the error over that range on its own.

A "trip" is one pass of the outermost grid-strided loop.  Where that loop is unrolled (colsum / BatchNorm: eight or four strides per pass and
a one-stride remainder loop) the shapes are chosen so that the unrolled body AND the remainder loop both run; per_trip is then the unrolled
pass where the entry says so.

Size budget: 40 M elements per case over all of its tensors, counted in fp32 units (bytes / 4): a bf16 tensor costs half.  With the literal
count the AdamW entry (w, g, m, v and the bf16 shadow of 2 * 4 194 304 parameters: 37.8 M units, 41.9 M tensor elements) could not hold two
full trips at all; the budget exists to bound memory and host time, which bytes do.  Entries whose fp32 form exceeds the budget run in bf16
storage only (a `shapes` table with the one key), and say why next to the entry.

Completeness -- every `gridDim` use and every cap helper in iseg_amd/csrc (searched: gridDim, cap_blocks, ew_blocks, row_blocks, lane_blocks,
eva_blocks, mc_blocks, rms_blocks, colsum_blocks, bn_blocks, bn_strip_blocks, ln_bwd_blocks, ln_any_bwd_blocks, grn_parts, bw_partitions
and the direct `grid_cap(items, per_block, cap)` grids; each helper is one grid_cap call of common.h with its own constants).

(a) IN THE TABLE (file: entry points)
  elementwise.hip  cast, scale_cols_cast, im2col (16-byte; scalar + zero_pad_cols; contiguous-run form), col2im (16-byte, scalar), colsum
                   (16-byte; scalar with a batch), broadcast_rows (store, accumulate), axpby, scale_dev, rowscale, dropout, fill_f32, act_fwd,
                   act_bwd, copy2d, add2d_f32, scale_rows_f32, layerscale_grads / layerscale_grads_slabs (gridDim.y strips)
  misc.hip         replace_nan_or_inf (min / max pass + apply pass), replace_nan_or_inf_bwd, rmsnorm_fwd / _bwd, pool2d_fwd, pool2d_bwd (scalar
                   form; arg-max + gather passes of the max-pool gradient), add_relu
  norm.hip         layernorm_fwd / _bwd (C = 96 in both lane splits, C = 8, any-width C = 5), layernorm_post_fwd / _bwd, layernorm_gather_fwd /
                   _bwd, bn_stats, bn_apply_fwd, bn_apply_fwd_packed, bn_bwd_reduce, bn_bwd_reduce_remask, bn_bwd_apply(_acc), bn_bwd_apply_remask
  resize.hip       resize_bilinear forward (row kernel, LDS-row kernel, 16-byte kernel), backward (LDS X pass, generic X pass scalar / 16-byte,
                   generic Y pass scalar / 16-byte, one-pass exact x2), align-corners forward / backward, resize_nearest_i32,
                   bn_relu_upsample_add
  attention.hip    clip_fwd / clip_bwd, gather_rows (16-byte, scalar), gather_rows_fma (window reverse + roll + residual, and its gradient),
                   softmax_rows_fwd / _bwd register kernels with 16 lanes per row, 64 x 2, 64 x 8 and 64 x 32; Swin's window partition / reverse
                   through backbones.swin.window_index_tables
  eva.hip          qkv_rope (in place, bf16), glu_fwd / glu_bwd scalar forms
  dcnv3.hip        mul_colsum (16-byte form at its 256 workgroups, scalar form at mc_blocks' 1024), scale_cols (scalar), split_cols_accumulate,
                   dcn_mask_softmax_fwd / _bwd
  loss.hip         softmax_ce_confusion (the persistent-tile form: taken when the confusion matrix rides along), argmax_confusion, upsample_ce
                   (gather kernel)
  mask_loss.hip    mask_loss_px_dice_kernel (the per-pixel route)
  gemm.hip:132     splitk_reduce_kernel, through gemm(split_k=2) with a bias
  grn.hip          grn_colsum_kernel strips (forward statistics and backward sums), grn_apply_kernel forward, grn_fold_weights
  dwconv.hip       dwconv_fwd_kernel through launch_fwd (forward and the flipped data-gradient form), dwconv_fwd_dma_kernel (persistent, three
                   rounds), dwconv_bwd_weight_lds_kernel
  defattn.hip      defattn_fwd (scalar form), defattn_bwd (4-lane form) with dcn_unfix_kernel behind it
  winattn.hip:356  win_bias_table_kernel (two full trips and 16 whole workgroups of a third: see BOUNDARY_OK)
  sod_metrics.hip:54  sod_minmax_kernel
  dwconv_strided.hip  dws_bwd_weight_kernel
  augment.hip      normalize_image, augment_crop_batch, augment_channel_means
  projective.hip   projective_transform_batch
  optim.hip        AdamW (adamw_kernel, grad_sq_blocks_kernel, grad_sq_segments_kernel), SGD (sgd_kernel, grad_sq_segments_kernel,
                   grad_sq_total_kernel over 601 variables)

(b) ALREADY PAST THE FIRST TRIP IN AN EXISTING TEST
  (none relied on: sod_minmax_kernel loops sixteen times at every size, but the existing normalize cases run it with one workgroup and extremes
  in every pass, so it has its own entry)

(c) GRID NOT CAPPED, CANNOT TAKE A SECOND TRIP (one workgroup / wavefront / thread per item: the grid grows with the problem)
  elementwise.hip  accumulate_pair (grid = ceil(2 n / 256), n a channel count: its loop body runs once), drop_path_mask(s), rsqrt_eps, transpose_batched,
                   layerscale_slabs_reduce_kernel's second job (one thread per four outputs)
  norm.hip         bn_finalize, ln_post_finish (one thread per channel)
  misc.hip         groupnorm_fwd / _bwd (one workgroup per (sample, group), block-strided inside)
  attention.hip    relpos_bias_gather / relpos_bias_scatter_grad (grid = ceil(total / 256); `int` index over heads x T x T table entries),
                   relpos_scatter_ws_kernel, colsum_wide (gridDim.y row chunks, each walks its own rows: no grid stride)
  loss.hip         softmax_ce_ignore / softmax_focal_ce_ignore WITHOUT a confusion matrix (grid = pixel tiles, the loop runs once), upsample_ce_kernel
                   (one wavefront per item), sum_blocks_kernel (one workgroup, thread-strided over the tile sums: 4134 of them in softmax_ce_confusion)
  mask_loss.hip    pass 1 / pass 2 (one workgroup per tile), finalize (one workgroup, thread-strided over B)
  mlp_fused.hip    mlp_prep / convnext_weight_prep_batched (grid = ceil(weight elements / 256)), the fused MLP kernels (one workgroup per row tile)
  gemm_impl.h, gemm_dma.h, dwconv_mfma.hip, dwconv_wgrad_mfma.hip, dwconv.hip:615,807  tile kernels: gridDim only feeds the XCD swizzle
  sod_metrics.hip:420, augment.hip:120, grn.hip:25  gridDim only indexes the partial buffer (blockIdx.y * gridDim.x + blockIdx.x): exercised by
                   the batched entries of (a) (augment_channel_means B = 2, grn_strips N = 2)
  winattn.hip:217  two windows per workgroup, grid = ceil(windows / 2)
  optim.hip        grad_sq_segments_kernel / grad_sq_total_kernel are single-workgroup, thread-strided loops: in (a) through the optimizer entries

(d) CAPPED, BUT TWO FULL TRIPS DO NOT FIT THE BUDGET IN ANY STORAGE TYPE, OR THE ROUTE IS SHADOWED
  attention.hip    softmax_fwd_kernel / softmax_bwd_kernel (the one-wavefront-per-row form, ld > 2048): one trip is 8192 x 4 rows x 2049 columns
                   = 67 M elements per tensor
  dcn_fixed.h      lane_blocks = 16384 x 256 lanes per trip.  dcn_unfix_kernel (one element per item) IS in (a) through defattn_bwd.  dcn_zero_kernel
                   clears 16 bytes per item: two trips are 134 MB of accumulators = 33.6 M units for 16.8 M gradient elements, whose value, dout and
                   dvalue add 25.2 M more in bf16 (it runs one full trip and a ragged second in the defattn entry).  The DCNv3 / DCNv2 sampling kernels
                   (dcnv3_fwd / _bwd / _bwd_gather, dcnv2_sample_*): a lane per (pixel, group, 8 channels) with 18 offsets and 9 mask values per
                   (pixel, group): 8.4 M lanes x (8 + 8 + 27) elements.  dcn_center_blend_fwd / _bwd and scale_cols' 16-byte form: 8.4 M lanes x 8
                   elements x >= 2 tensors
  eva.hip          the 16-byte forms of glu_fwd / glu_bwd and qkv_rope out of place: 8.4 M items of 8 elements x >= 2 tensors
  dwconv_strided.hip  dws_fwd_kernel / dws_bwd_data_kernel: 16384 x 256 items of 8 channels, 67 M elements per tensor
  grn.hip          grn_apply_kernel backward: 3 tensors x 33.6 M elements (its forward instantiation is in (a) in bf16)
  norm.hip         layernorm_bwd at ln_bwd_blocks' cap of 1024 in fp32 storage (3 x 25.2 M; in (a) in bf16, and below the cap in fp32)
  dwconv.hip:642   dwconv_bwd_weight_dma_kernel (bf16, C % 32 == 0, at most 512 / slabs workgroups over N x ceil(H / 8) x ceil(W / 32) tiles): from 768
                   units of 16 x 16 x 16 channels on, iseg_dwconv2d_bwd_weight takes the matrix-core kernel instead; below that a C = 32 plane has
                   fewer than 384 x 4 / 3 = 512 tiles, i.e. never more than one per workgroup.  dwconv_bwd_weight_kernel (:305, the register form)
                   splits its items by a per-workgroup count and has no grid stride
"""
from collections import namedtuple

Trip = namedtuple("Trip", "grid per_trip items quantum tail")
Case = namedtuple("Case", "name wrapper source cap launcher shapes elements")      # shapes: {"f32": {...}, "bf16": {...}} (one key: that storage only)

BUDGET = 40_000_000      # fp32 units (bytes / 4) per case
BYTES = {"f32": 4, "bf16": 2}


def cdiv(a, b):
    return -(-a // b)


def capped(blocks, cap):
    return max(1, min(cap, blocks))


def trip(grid, per_block, items, tail=None):
    return Trip(grid, grid * per_block, items, per_block, tail)


def first_of_last_trip(t):
    return t.items // t.per_trip * t.per_trip


# entries whose item count is by construction a multiple of the workgroup quantum: the third trip is partial in whole workgroups
BOUNDARY_OK = {"win_bias_table": "nW x heads x 64 x 64 table entries: a multiple of 4096 = 16 workgroups of 256"}


def violations(t, boundary_ok=False):
    """the two-full-trips-plus-a-ragged-third rule; returns the list of broken clauses"""
    bad = []
    if not t.items > 2 * t.per_trip:
        bad.append(f"items {t.items} <= 2 * per_trip {t.per_trip}")
    rem = t.items % t.per_trip
    if rem == 0:
        bad.append("no ragged trip")
    elif t.quantum > 1 and rem % t.quantum == 0 and not boundary_ok:
        bad.append(f"ragged trip {rem} ends on a workgroup boundary ({t.quantum})")
    if t.tail is not None and t.tail == 0:
        bad.append("no scalar tail")
    return bad


def units(dtype, *counts, f32=0, other_bytes=0):
    """fp32 units of `counts` elements in the storage type plus `f32` fp32 elements plus raw bytes"""
    return (sum(counts) * BYTES[dtype] + f32 * 4 + other_bytes) // 4


# ------------------------------------------------------------------------------------------------------------------------------------
# elementwise.hip: cap_blocks(work, 256) = min(2048, ceil(work / 256)) workgroups of 256 lanes
# ------------------------------------------------------------------------------------------------------------------------------------
def ew_cap_blocks(work):
    return capped(cdiv(work, 256), 2048)


def ew_vec8(n):
    """cast / axpby / scale_dev / dropout / act: 8 elements per lane, then a scalar tail"""
    return trip(ew_cap_blocks(cdiv(n, 8)), 256, n // 8, tail=n % 8)


def ew_items(items):
    return trip(ew_cap_blocks(items), 256, items)


N_EW = 2 * 4_194_304 + 8 * 300 + 5          # two trips of 2048 * 256 lanes of 8, 300 more lanes, a 5-element tail
R_EW = N_EW // 8                            # the same lane count as rows of C = 8
SC_ROWS, SC_COLS = 1300, 1009               # scalar-indexed kernels: 1 311 700 elements against 524 288 per trip
IM_HW = 1026                                # 2 x 2 stride 2 on 1026 x 1026: M = 513 * 513 = 263 169 output pixels


def both(**shape):
    return {"f32": dict(shape), "bf16": dict(shape)}


def only(dtype, **shape):
    return {dtype: dict(shape)}


def _im2col(dtype, N, H, W, C, K, s, ldc):
    Ho, Wo = H // s, W // s
    M = N * Ho * Wo
    vec = C % 8 == 0 and ldc % 8 == 0
    runs = not vec and (K * C) % 4 == 0 and ldc % 4 == 0 and (W * C) % 4 == 0 and (s * C) % 4 == 0
    items = M * K * (K * C // 4) if runs else M * K * K * (C // 8 if vec else C)
    trips = [ew_items(items)]
    if ldc > K * K * C:
        trips.append(ew_items(M * (ldc - K * K * C)))      # zero_pad_cols_kernel
    return trips


def _colsum(dtype, batch, rows, C):
    V = 8 if C % 8 == 0 else 1
    nch = C // V
    tpc = min(nch, 256)
    rpi = 256 // tpc
    grid = capped(cdiv(rows, rpi * 8), 256)
    # V = 8: eight strides per pass of the unrolled loop, then the one-stride remainder loop; V = 1: the one-stride loop only
    return [trip(grid, rpi * (8 if V == 8 else 1), rows)]


# ------------------------------------------------------------------------------------------------------------------------------------
# misc.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def misc_ew_blocks(n):
    return capped(cdiv(n, 256), 4096)


def _sanitize(dtype, n):
    return [trip(capped(cdiv(cdiv(n, 8), 256), 1024), 256, n // 8, tail=n % 8),      # finite_minmax_kernel
            trip(misc_ew_blocks(n), 256, n // 8, tail=n % 8)]                      # sanitize_apply_kernel (grid sized by n, loop over n / 8)


def _rms(dtype, rows, C):
    return [trip(capped(cdiv(rows, 32), 512), 4, rows)]


N_SAN = 2 * 8_388_608 + 8 * 300 + 5
POOL = dict(N=1, H=2000, W=1402, C=3, k=3, s=2)      # SAME: Ho = 1000, Wo = 701


def _pool_fwd(dtype, N, H, W, C, k, s):
    return [trip(misc_ew_blocks(N * cdiv(H, s) * cdiv(W, s) * C), 256, N * cdiv(H, s) * cdiv(W, s) * C)]


def _pool_bwd(dtype, N, H, W, C, k, s):
    return [trip(misc_ew_blocks(N * H * W * C), 256, N * H * W * C)]


# ------------------------------------------------------------------------------------------------------------------------------------
# norm.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def ln_lanes_per_row(C, thirds=False):
    chunks = cdiv(C, 8)
    if thirds and chunks % 3 == 0 and chunks <= 24:
        t = chunks // 3
        if t >= 1 and t & (t - 1) == 0:
            return t
    lanes = 1
    while lanes < chunks and lanes < 64:
        lanes <<= 1
    return lanes


def _ln_fwd(dtype, rows, C):
    if C % 8:
        return [trip(capped(cdiv(rows, 4), 2048), 4, rows)]
    rpw = 64 // ln_lanes_per_row(C, dtype == "bf16")
    return [trip(capped(cdiv(rows, rpw * 4), 2048), rpw * 4, rows)]


def ln_bwd_blocks(rows, C):
    rpw = 64 // ln_lanes_per_row(C)
    rows_per_block = max(24576 // C, rpw * 4)
    blocks = cdiv(rows, rows_per_block)
    if blocks < 256:
        blocks = min(cdiv(rows, rpw * 4), 256)
    return capped(blocks, 1024)


def _ln_bwd(dtype, rows, C):
    if C % 8:
        return [trip(capped(cdiv(rows, 8), 512), 2, rows)]      # LN_ANY_WAVES = 2 rows per workgroup and pass
    lpr = ln_lanes_per_row(C)
    cpl = cdiv(C // 8, lpr)
    U = (4 if lpr >= 32 else 2 if lpr >= 16 else 1) if cpl <= 1 else 4 if cpl <= 2 else 2 if cpl <= 4 else 1
    return [trip(ln_bwd_blocks(rows, C), 4 * (64 // lpr) * U, rows)]


def _ln_fwd_bwd(dtype, rows, C):
    return _ln_fwd(dtype, rows, C) + _ln_bwd(dtype, rows, C)


def _bn_rpi(C):
    return 256 // min(C // 8, 256)


def _bn_stats(dtype, rows, C):
    return [trip(capped(cdiv(rows, _bn_rpi(C) * 4), 256), _bn_rpi(C), rows)]


def _bn_reduce(dtype, rows, C):
    return [trip(capped(cdiv(rows, _bn_rpi(C) * 4), 1024), _bn_rpi(C), rows)]


def _bn_strip(dtype, rows, C):
    return [trip(capped(cdiv(rows, _bn_rpi(C) * 8), 4096), _bn_rpi(C), rows)]


LN96_CAP = 2 * (2048 * 64) + 37             # bf16 forward: 4 lanes per row, 64 rows per workgroup; also > 1023 * 256: ln_bwd_blocks = 1024
LN96_F32 = 2 * (2048 * 16) + 37             # fp32 forward: 16 lanes per row, 16 rows per workgroup; backward 257 workgroups x 32 rows
LN8 = 2 * (2048 * 256) + 37
LN5 = 2 * 8192 + 37
BN_STATS_ROWS = 9 * 65536 + 256 * 37 + 5            # stride 256 * 256 rows: one pass of the 8-stride body, then the remainder loop
BN_REDUCE_ROWS = 5 * 262144 + 256 * 37 + 5          # stride 1024 * 256 rows: one pass of the 4-stride body, then the remainder loop
BN_STRIP_ROWS = 2 * 1048576 + 256 * 37 + 5          # stride 4096 * 256 rows (remainder loop only)
BN_STRIP_ROWS_UNROLLED = 4 * 1048576 + 256 * 37 + 5  # ... and one pass of the 4-stride body (bf16: fits the budget)


# ------------------------------------------------------------------------------------------------------------------------------------
# resize.hip: its own cap_blocks(items) = min(2048, ceil(items / 256)); row grids min(4096, N Ho) forward, min(2048, N Ho) backward
# ------------------------------------------------------------------------------------------------------------------------------------
def _rs_fwd(dtype, N, Hi, Wi, Ho, Wo, C):
    lds = (2 * Wi * C + 3 * Wo) * 4
    if lds <= 48 * 1024 and Wo * C >= 1024:
        return [Trip(capped(N * Ho, 4096), capped(N * Ho, 4096), N * Ho, 1, None)]       # resize_bilinear_fwd_lds_kernel
    if C % 8 == 0:
        return [ew_items(N * Ho * Wo * (C // 8))]                                        # resize_bilinear_fwd_vec_kernel
    return [Trip(capped(N * Ho, 4096), capped(N * Ho, 4096), N * Ho, 1, None)]           # resize_bilinear_fwd_kernel


def _rs_fwd_ac(dtype, N, Hi, Wi, Ho, Wo, C):
    return [Trip(capped(N * Ho, 4096), capped(N * Ho, 4096), N * Ho, 1, None)]


def _rs_bwd(dtype, N, Hi, Wi, Ho, Wo, C, cross):
    """`cross`: which pass the shape is chosen for ("x2", "x", "y"); the other pass of a two-pass shape may stay inside one trip"""
    if Ho == 2 * Hi and Wo == 2 * Wi and C % 8 == 0:
        return [ew_items(N * Hi * Wi * (C // 8))]
    row_bytes = (Wo * C + 3 * Wo) * 4
    if row_bytes <= 64 * 1024:
        xp = Trip(capped(N * Ho, 2048), capped(N * Ho, 2048), N * Ho, 1, None)
    elif C % 8 == 0:
        xp = ew_items(N * Ho * Wi * C // 8)
    else:
        xp = ew_items(N * Ho * Wi * C)
    yp = ew_items(N * Hi * Wi * C // 8) if (Wi * C) % 8 == 0 else ew_items(N * Hi * Wi * C)
    return [xp if cross == "x" else yp]


def _rs_bwd_ac(dtype, N, Hi, Wi, Ho, Wo, C):
    return [ew_items(N * Ho * Wi * C), ew_items(N * Hi * Wi * C)]


def _bn_up_add(dtype, N, Hi, Wi, Ho, Wo, C):
    rpi = 256 // min(C // 8, 256)
    return [trip(capped(cdiv(N * Ho * Wo, rpi * 4), 4096), rpi, N * Ho * Wo)]


# ------------------------------------------------------------------------------------------------------------------------------------
# attention.hip: ew_blocks(n) = min(4096, ceil(n / 256)), row_blocks(rows) = min(8192, ceil(rows / 4))
# ------------------------------------------------------------------------------------------------------------------------------------
N_CLIP = 2 * 1_048_576 + 256 * 18 + 5


def _att_ew(dtype, n):
    return [trip(misc_ew_blocks(n), 256, n)]


def _gather_rows(dtype, rows, C):
    V = {"f32": 4, "bf16": 8}[dtype] if (C * BYTES[dtype]) % 16 == 0 else 1
    return [trip(misc_ew_blocks(rows * (C // V)), 256, rows * (C // V))]


def _gather_fma(dtype, rows, C, res):
    return [trip(misc_ew_blocks(rows * (C // 8)), 256, rows * (C // 8))]


def _softmax_reg(dtype, rows, ld):
    lpr = 16 if ld <= 16 else 64
    rpw = 64 // lpr
    return [trip(capped(cdiv(cdiv(rows, rpw), 4), 8192), 4 * rpw, rows)]


# ------------------------------------------------------------------------------------------------------------------------------------
# eva.hip: eva_blocks(work) = min(16384, ceil(work / 256));  dcn_fixed.h: lane_blocks(n) = the same cap;  others as named
# ------------------------------------------------------------------------------------------------------------------------------------
def lane_blocks(n):
    return capped(cdiv(n, 256), 16384)


def lanes(items):
    return trip(lane_blocks(items), 256, items)


N_LANE = 2 * 4_194_304 + 256 * 5 + 117       # scalar (one element per item) kernels under the 16384-workgroup caps
ROPE = dict(B=399_501, tokens=7, prefix=1, C=8, hd=8)      # 2 796 507 rows of 3 C / 8 = 3 pieces
MC_VEC_ROWS = 5 * 65536 + 256 * 37 + 5       # mul_colsum 16-byte form: 256 workgroups x 256 row lanes; one pass of the 4-stride body + remainder loop
GRN_STRIP = dict(N=2, HW=5 * 65536 + 256 * 37 + 5, C=8)
GRN_APPLY = dict(N=2, HW=2_097_300, C=8)


def _grn_parts(N, HW, C):
    rpi = 256 // min(C // 8, 256)
    return capped(min(cdiv(HW, rpi * 8), 1 if N >= 2048 else 2048 // N), 256), rpi


def _grn(dtype, N, HW, C):
    P, rpi = _grn_parts(N, HW, C)
    return [trip(P, rpi, HW), trip(capped(cdiv(N * HW * (C // 8), 256), 8192), 256, N * HW * (C // 8))]


def _dw_fwd(dtype, N, H, W, C, K, dil):
    tiles = N * H * cdiv(W, 4)              # TW = 4 output columns per lane tile; gs = 1 channel group at C = 8: 256 tiles per workgroup and pass
    return [trip(capped(cdiv(tiles, 256), 2048), 256, tiles)]


# ------------------------------------------------------------------------------------------------------------------------------------
# optim.hip: min(4096, nblocks) workgroups; AdamW / the block norms take 4 blocks of 256 parameters per workgroup and pass, SGD one
# ------------------------------------------------------------------------------------------------------------------------------------
def opt_variables(total, big, count):
    """sizes of the variables of an optimizer case: element counts, each padded to a 256-block by ParamStore"""
    rest = total - big
    small = count - 1
    each = rest // small
    sizes = [big] + [each] * (small - 1)
    sizes.append(rest - each * (small - 1))
    return sizes


def _opt_blocks(sizes):
    return sum(cdiv(s, 256) for s in sizes)


def _adamw(dtype, total, big, count, clip):
    nb = _opt_blocks(opt_variables(total, big, count))
    g = capped(nb, 4096)
    trips = [trip(g, 4, nb)]                                            # adamw_kernel
    if clip:
        trips.append(trip(g, 4, nb))                                    # grad_sq_blocks_kernel
        trips.append(trip(1, 256, cdiv(big, 256)))             # grad_sq_segments_kernel: 256 lanes over the blocks of the big variable
        if clip == "global_clipnorm":
            trips.append(trip(1, 256, count))                  # grad_sq_total_kernel: 256 lanes over the variables
    return trips


def _sgd(dtype, total, big, count, clip):
    nb = _opt_blocks(opt_variables(total, big, count))
    trips = [trip(capped(nb, 4096), 1, nb)]                             # sgd_kernel (grad_sq_blocks stays inside one trip here: the AdamW case drives it)
    if clip:
        trips.append(trip(1, 256, cdiv(big, 256)))
        if clip == "global_clipnorm":
            trips.append(trip(1, 256, count))
    return trips


ADAMW_N = 2 * 4_194_304 + 256 * 7 + 3
SGD_N = 2 * 1_048_576 + 256 * 5 + 3
OPT_BIG = 2 * 65536 + 256 * 300 + 77      # > 65 536 * 2 elements: 813 blocks, the 256-lane segment loop runs 3 full passes + 45


CASES = [
    # ---- elementwise.hip ------------------------------------------------------------------------------------------------------------
    Case("cast", "kernels.cast", "elementwise.hip:iseg_cast", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW),
         lambda d, n: units(d, n) + n),      # f32 -> storage type and back: one fp32 tensor + one of the storage type per direction
    Case("scale_cols_cast", "kernels.scale_cols_cast", "elementwise.hip:iseg_scale_cols_cast", "cap_blocks 2048",
         lambda d, rows, cols: [ew_items(rows * cols)], both(rows=SC_ROWS, cols=SC_COLS), lambda d, rows, cols: units(d, rows * cols, f32=rows * cols)),
    Case("im2col_vec", "kernels.im2col", "elementwise.hip:iseg_im2col (im2col_kernel<8>)", "cap_blocks 2048", _im2col,
         both(N=1, H=IM_HW, W=IM_HW, C=8, K=2, s=2, ldc=32), lambda d, N, H, W, C, K, s, ldc: units(d, N * H * W * C, N * (H // s) * (W // s) * ldc)),
    Case("im2col_scalar_and_pad", "kernels.im2col", "elementwise.hip:iseg_im2col (im2col_kernel<1>, zero_pad_cols_kernel)", "cap_blocks 2048", _im2col,
         both(N=1, H=IM_HW, W=IM_HW, C=3, K=2, s=2, ldc=16), lambda d, N, H, W, C, K, s, ldc: units(d, N * H * W * C, N * (H // s) * (W // s) * ldc)),
    Case("im2col_runs", "kernels.im2col", "elementwise.hip:iseg_im2col (im2col_runs_kernel)", "cap_blocks 2048", _im2col,
         both(N=1, H=1188, W=1188, C=3, K=4, s=4, ldc=48), lambda d, N, H, W, C, K, s, ldc: units(d, N * H * W * C, N * (H // s) * (W // s) * ldc)),
    Case("col2im_vec", "kernels.col2im", "elementwise.hip:iseg_col2im (col2im_kernel<8>)", "cap_blocks 2048",
         lambda d, N, H, W, C, K, s, ldc: [ew_items(N * H * W * (C // 8))], both(N=1, H=IM_HW, W=IM_HW, C=8, K=2, s=2, ldc=32),
         lambda d, N, H, W, C, K, s, ldc: units(d, N * H * W * C, N * (H // s) * (W // s) * ldc)),
    Case("col2im_scalar", "kernels.col2im", "elementwise.hip:iseg_col2im (col2im_kernel<1>)", "cap_blocks 2048",
         lambda d, N, H, W, C, K, s, ldc: [ew_items(N * H * W * C)], both(N=1, H=IM_HW, W=IM_HW, C=3, K=2, s=2, ldc=16),
         lambda d, N, H, W, C, K, s, ldc: units(d, N * H * W * C, N * (H // s) * (W // s) * ldc)),
    Case("colsum_vec", "kernels.colsum", "elementwise.hip:iseg_colsum (colsum_partial_kernel<8>)", "colsum_blocks 256", _colsum,
         both(batch=1, rows=2 * (256 * 256 * 8) + 256 * 37 + 5, C=8), lambda d, batch, rows, C: units(d, batch * rows * C)),
    Case("colsum_scalar_batched", "kernels.colsum", "elementwise.hip:iseg_colsum (colsum_partial_kernel<1>, blockIdx.y = sample)", "colsum_blocks 256",
         _colsum, both(batch=2, rows=2 * (256 * 85 * 8) + 85 * 37 + 5, C=3), lambda d, batch, rows, C: units(d, batch * rows * C)),
    Case("broadcast_rows", "kernels.broadcast_rows", "elementwise.hip:iseg_broadcast_rows (store and accumulate)", "cap_blocks 2048",
         lambda d, B, R, C: [ew_items(B * R * (C // 8))], both(B=2, R=R_EW // 2, C=8), lambda d, B, R, C: units(d, B * R * C)),
    Case("axpby", "kernels.axpby", "elementwise.hip:iseg_axpby", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW), lambda d, n: units(d, 3 * n)),
    Case("scale_dev", "kernels.scale_dev", "elementwise.hip:iseg_scale_dev", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW),
         lambda d, n: units(d, 2 * n)),
    Case("rowscale", "kernels.rowscale", "elementwise.hip:iseg_rowscale", "cap_blocks 2048", lambda d, rows, C, rpg: [ew_items(rows * (C // 8))],
         both(rows=R_EW, C=8, rpg=400_000), lambda d, rows, C, rpg: units(d, 2 * rows * C)),
    Case("dropout", "kernels.dropout", "elementwise.hip:iseg_dropout", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW),
         lambda d, n: units(d, 2 * n)),
    Case("fill_f32", "kernels.fill_f32", "elementwise.hip:iseg_fill_f32", "cap_blocks 2048", lambda d, n: [ew_items(n)], only("f32", n=SC_ROWS * SC_COLS),
         lambda d, n: n),
    Case("act_fwd", "kernels.act_fwd", "elementwise.hip:iseg_act_fwd", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW), lambda d, n: units(d, 2 * n)),
    Case("act_bwd", "kernels.act_bwd", "elementwise.hip:iseg_act_bwd", "cap_blocks 2048", lambda d, n: [ew_vec8(n)], both(n=N_EW), lambda d, n: units(d, 3 * n)),
    Case("copy2d", "kernels.copy2d", "elementwise.hip:iseg_copy2d", "cap_blocks 2048", lambda d, rows, cols, lds, ldd: [ew_items(rows * (cols // 8))],
         both(rows=R_EW, cols=8, lds=16, ldd=8), lambda d, rows, cols, lds, ldd: units(d, rows * lds, rows * ldd)),
    Case("add2d_f32", "kernels.add2d", "elementwise.hip:iseg_add2d_f32", "cap_blocks 2048", lambda d, rows, cols, lds, ldd: [ew_items(rows * cols)],
         only("f32", rows=SC_ROWS, cols=SC_COLS, lds=SC_COLS + 3, ldd=SC_COLS + 7), lambda d, rows, cols, lds, ldd: rows * (lds + ldd)),
    Case("scale_rows_f32", "kernels.scale_rows", "elementwise.hip:iseg_scale_rows_f32", "cap_blocks 2048", lambda d, rows, C: [ew_items(rows * C)],
         only("f32", rows=SC_ROWS, C=SC_COLS), lambda d, rows, C: 2 * rows * C),
    # ---- misc.hip -------------------------------------------------------------------------------------------------------------------
    Case("replace_nan_or_inf", "kernels.replace_nan_or_inf", "misc.hip:iseg_replace_nan_or_inf (finite_minmax_kernel 1024, sanitize_apply_kernel ew_blocks)",
         "1024 / ew_blocks 4096", _sanitize, both(n=N_SAN), lambda d, n: units(d, 2 * n)),
    Case("replace_nan_or_inf_bwd", "kernels.replace_nan_or_inf_bwd", "misc.hip:iseg_replace_nan_or_inf_bwd", "ew_blocks 4096",
         lambda d, n: [trip(misc_ew_blocks(n), 256, n // 8, tail=n % 8)], only("bf16", n=N_SAN), lambda d, n: units(d, 3 * n)),      # fp32: 50 M
    Case("rmsnorm", "kernels.rmsnorm_fwd / rmsnorm_bwd", "misc.hip:iseg_rmsnorm_fwd / iseg_rmsnorm_bwd", "rms_blocks 512",
         lambda d, rows, C: _rms(d, rows, C) * 2, both(rows=32805, C=8), lambda d, rows, C: units(d, 4 * rows * C)),
    Case("pool2d_fwd", "kernels.pool2d_fwd", "misc.hip:iseg_pool2d_fwd", "ew_blocks 4096", _pool_fwd, both(**POOL),
         lambda d, N, H, W, C, k, s: units(d, N * H * W * C, N * cdiv(H, s) * cdiv(W, s) * C)),
    Case("pool2d_bwd_scalar", "kernels.pool2d_bwd", "misc.hip:iseg_pool2d_bwd (pool2d_bwd_kernel)", "ew_blocks 4096", _pool_bwd, both(**POOL),
         lambda d, N, H, W, C, k, s: units(d, 2 * N * H * W * C, N * cdiv(H, s) * cdiv(W, s) * C)),
    Case("add_relu", "kernels.add_relu", "misc.hip:iseg_add_relu", "ew_blocks 4096", lambda d, n: [trip(misc_ew_blocks(n // 8), 256, n // 8)],
         only("bf16", n=N_SAN - 5), lambda d, n: units(d, 3 * n)),      # fp32: 50 M
    # ---- norm.hip -------------------------------------------------------------------------------------------------------------------
    Case("layernorm_fwd_c96", "kernels.layernorm_fwd", "norm.hip:layernorm_fwd_launch (bf16: 4 lanes per row, fp32: 16)", "2048", _ln_fwd,
         {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)}, lambda d, rows, C: units(d, 2 * rows * C)),
    Case("layernorm_bwd_c96", "kernels.layernorm_bwd", "norm.hip:layernorm_bwd_launch (ln_bwd_blocks: 1024 in bf16, 257 below the cap in fp32)",
         "ln_bwd_blocks 1024", _ln_bwd, {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)},      # fp32 at the cap: 3 x 25.2 M
         lambda d, rows, C: units(d, 3 * rows * C)),
    Case("layernorm_fwd_c8", "kernels.layernorm_fwd", "norm.hip:layernorm_fwd_launch (one lane per row)", "2048", _ln_fwd, both(rows=LN8, C=8),
         lambda d, rows, C: units(d, 2 * rows * C)),
    Case("layernorm_bwd_c8", "kernels.layernorm_bwd", "norm.hip:layernorm_bwd_launch (ln_bwd_blocks = 342, eleven passes)", "ln_bwd_blocks", _ln_bwd,
         both(rows=LN8, C=8), lambda d, rows, C: units(d, 4 * rows * C)),
    Case("layernorm_fwd_any_c5", "kernels.layernorm_fwd", "norm.hip:layernorm_fwd_any_kernel", "2048", _ln_fwd, both(rows=LN5, C=5),
         lambda d, rows, C: units(d, 2 * rows * C)),
    Case("layernorm_bwd_any_c5", "kernels.layernorm_bwd", "norm.hip:layernorm_bwd_any_kernel (ln_any_bwd_blocks)", "ln_any_bwd_blocks 512", _ln_bwd,
         both(rows=LN5, C=5), lambda d, rows, C: units(d, 4 * rows * C)),
    Case("layernorm_post_fwd", "kernels.layernorm_post_fwd", "norm.hip:iseg_layernorm_post_fwd (layernorm_fwd_kernel<POST>)", "2048", _ln_fwd,
         {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)}, lambda d, rows, C: units(d, 3 * rows * C)),
    Case("layernorm_post_bwd", "kernels.layernorm_post_bwd", "norm.hip:iseg_layernorm_post_bwd (layernorm_bwd_kernel<POST>)", "ln_bwd_blocks 1024", _ln_bwd,
         {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)}, lambda d, rows, C: units(d, 3 * rows * C)),
    Case("layernorm_gather_fwd", "kernels.layernorm_gather_fwd", "norm.hip:iseg_layernorm_gather_fwd (rows = OUTPUT rows)", "2048", _ln_fwd,
         {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)}, lambda d, rows, C: units(d, 2 * rows * C)),
    Case("layernorm_gather_bwd", "kernels.layernorm_gather_bwd", "norm.hip:iseg_layernorm_gather_bwd (rows = SOURCE rows)", "ln_bwd_blocks 1024", _ln_bwd,
         {"f32": dict(rows=LN96_F32, C=96), "bf16": dict(rows=LN96_CAP, C=96)},
         lambda d, rows, C: units(d, 3 * rows * C + cdiv(rows, 16) * C)),      # dy has one padding row per 16 source rows
    Case("bn_stats", "kernels.bn_stats", "norm.hip:iseg_bn_stats (bn_blocks 256)", "bn_blocks 256", _bn_stats, both(rows=BN_STATS_ROWS, C=8),
         lambda d, rows, C: units(d, rows * C)),
    Case("bn_apply_fwd", "kernels.bn_apply_fwd", "norm.hip:iseg_bn_apply_fwd (bn_strip_blocks 4096)", "bn_strip_blocks 4096", _bn_strip,
         {"f32": dict(rows=BN_STRIP_ROWS, C=8), "bf16": dict(rows=BN_STRIP_ROWS_UNROLLED, C=8)}, lambda d, rows, C: units(d, 2 * rows * C)),
    Case("bn_apply_fwd_packed", "kernels.bn_finalize_apply", "norm.hip:iseg_bn_apply_fwd_packed (bn_strip_blocks 4096)", "bn_strip_blocks 4096", _bn_strip,
         {"f32": dict(rows=BN_STRIP_ROWS, C=8), "bf16": dict(rows=BN_STRIP_ROWS_UNROLLED, C=8)}, lambda d, rows, C: units(d, 2 * rows * C)),
    Case("bn_bwd_reduce", "kernels.bn_bwd_reduce", "norm.hip:iseg_bn_bwd_reduce (bn_blocks 1024)", "bn_blocks 1024", _bn_reduce,
         both(rows=BN_REDUCE_ROWS, C=8), lambda d, rows, C: units(d, 3 * rows * C)),
    Case("bn_bwd_reduce_remask", "kernels.bn_bwd_reduce_remask", "norm.hip:iseg_bn_bwd_reduce_remask (bn_blocks 1024)", "bn_blocks 1024", _bn_reduce,
         both(rows=BN_REDUCE_ROWS, C=8), lambda d, rows, C: units(d, 2 * rows * C)),
    Case("bn_bwd_apply", "kernels.bn_bwd_apply", "norm.hip:iseg_bn_bwd_apply_acc (bn_strip_blocks 4096)", "bn_strip_blocks 4096", _bn_strip,
         only("bf16", rows=BN_STRIP_ROWS, C=8), lambda d, rows, C: units(d, 4 * rows * C)),      # fp32: 4 x 16.9 M
    Case("bn_bwd_apply_remask", "kernels.bn_bwd_apply_remask", "norm.hip:iseg_bn_bwd_apply_remask (bn_strip_blocks 4096)", "bn_strip_blocks 4096", _bn_strip,
         only("bf16", rows=BN_STRIP_ROWS, C=8), lambda d, rows, C: units(d, 3 * rows * C)),      # fp32: 3 x 16.9 M
    # ---- resize.hip -----------------------------------------------------------------------------------------------------------------
    Case("resize_fwd_rows", "kernels.resize_bilinear", "resize.hip:iseg_resize_bilinear_fwd (resize_bilinear_fwd_kernel, row grid)", "4096 rows", _rs_fwd,
         both(N=2, Hi=5, Wi=3, Ho=4100, Wo=4, C=3), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C, f32=N * Ho * Wo * C)),
    Case("resize_fwd_lds_rows", "kernels.resize_bilinear", "resize.hip:iseg_resize_bilinear_fwd (resize_bilinear_fwd_lds_kernel, row grid)", "4096 rows", _rs_fwd,
         both(N=2, Hi=5, Wi=3, Ho=4100, Wo=342, C=3), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C, f32=N * Ho * Wo * C)),
    Case("resize_fwd_vec", "kernels.resize_bilinear", "resize.hip:iseg_resize_bilinear_fwd (resize_bilinear_fwd_vec_kernel)", "cap_blocks 2048", _rs_fwd,
         both(N=2, Hi=7, Wi=5, Ho=4200, Wo=127, C=8), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C, N * Ho * Wo * C)),
    Case("resize_bwd_x_lds_rows", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (resize_bwd_x_lds_kernel, row grid)", "2048 rows",
         lambda d, **s: _rs_bwd(d, cross="x", **s), both(N=2, Hi=5, Wi=3, Ho=4100, Wo=4, C=3),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, 2 * N * Hi * Wi * C, f32=N * Ho * Wo * C + N * Ho * Wi * C)),
    Case("resize_bwd_x_scalar", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (X pass, resize_bwd_axis_kernel)", "cap_blocks 2048",
         lambda d, **s: _rs_bwd(d, cross="x", **s), both(N=1, Hi=2440, Wi=87, Ho=2440, Wo=2049, C=5),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    Case("resize_bwd_x_vec", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (X pass, resize_bwd_axis_vec_kernel)", "cap_blocks 2048",
         lambda d, **s: _rs_bwd(d, cross="x", **s), both(N=1, Hi=1030, Wi=1021, Ho=1030, Wo=1500, C=8),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    Case("resize_bwd_y_scalar", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (Y pass, resize_bwd_axis_kernel)", "cap_blocks 2048",
         lambda d, **s: _rs_bwd(d, cross="y", **s), both(N=2, Hi=700, Wi=251, Ho=350, Wo=125, C=3),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, 2 * N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    Case("resize_bwd_y_vec", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (Y pass, resize_bwd_axis_vec_kernel)", "cap_blocks 2048",
         lambda d, **s: _rs_bwd(d, cross="y", **s), both(N=2, Hi=1030, Wi=511, Ho=515, Wo=3, C=8),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, 2 * N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    Case("resize_bwd_x2", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (resize_bwd_x2_vec_kernel)", "cap_blocks 2048",
         lambda d, **s: _rs_bwd(d, cross="x2", **s), only("bf16", N=2, Hi=1030, Wi=511, Ho=2060, Wo=1022, C=8),      # fp32: 41.9 M
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C + N * Ho * Wo * C)),
    Case("resize_ac_fwd_rows", "kernels.resize_bilinear(align_corners=True)", "resize.hip:iseg_resize_bilinear_ac_fwd (row grid)", "4096 rows", _rs_fwd_ac,
         both(N=2, Hi=5, Wi=3, Ho=4100, Wo=4, C=3), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C, f32=N * Ho * Wo * C)),
    Case("resize_ac_bwd", "kernels.resize_bilinear_bwd(align_corners=True)", "resize.hip:iseg_resize_bilinear_ac_bwd (both passes)", "cap_blocks 2048", _rs_bwd_ac,
         both(N=2, Hi=700, Wi=251, Ho=701, Wo=4, C=3), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, 2 * N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    Case("resize_nearest_i32", "kernels.resize_nearest_i32", "resize.hip:iseg_resize_nearest_i32", "cap_blocks 2048",
         lambda d, N, Hi, Wi, Ho, Wo, C: [ew_items(N * Ho * Wo * C)], only("f32", N=2, Hi=37, Wi=29, Ho=4100, Wo=43, C=3),
         lambda d, N, Hi, Wi, Ho, Wo, C: N * Hi * Wi * C + N * Ho * Wo * C),
    Case("bn_relu_upsample_add", "kernels.bn_relu_upsample_add", "resize.hip:iseg_bn_relu_upsample_add", "4096", _bn_up_add,
         both(N=1, Hi=513, Wi=1029, Ho=1026, Wo=2058, C=8), lambda d, N, Hi, Wi, Ho, Wo, C: units(d, N * Hi * Wi * C + 2 * N * Ho * Wo * C)),
    # ---- attention.hip --------------------------------------------------------------------------------------------------------------
    Case("clip_fwd_bwd", "kernels.clip_fwd / clip_bwd", "attention.hip:iseg_clip_fwd / iseg_clip_bwd", "ew_blocks 4096", lambda d, n: _att_ew(d, n) * 2,
         both(n=N_CLIP), lambda d, n: units(d, 3 * n)),
    Case("gather_rows_vec", "kernels.gather_rows", "attention.hip:iseg_gather_rows (16-byte chunks)", "ew_blocks 4096", _gather_rows,
         both(rows=N_CLIP, C=8), lambda d, rows, C: units(d, 2 * rows * C, f32=rows)),
    Case("gather_rows_scalar", "kernels.gather_rows", "attention.hip:iseg_gather_rows (scalar)", "ew_blocks 4096", _gather_rows,
         both(rows=N_CLIP // 3, C=3), lambda d, rows, C: units(d, 2 * rows * C, f32=rows)),
    Case("gather_rows_fma", "kernels.gather_rows_fma", "attention.hip:iseg_gather_rows_fma (window reverse + roll + residual; its gradient)", "ew_blocks 4096",
         _gather_fma, {"f32": dict(rows=N_CLIP, C=8, res=0), "bf16": dict(rows=N_CLIP, C=8, res=1)},      # fp32 with the residual: 3 x 16.8 M
         lambda d, rows, C, res: units(d, (2 + res) * rows * C, f32=rows)),
    Case("softmax_rows_16", "kernels.softmax_rows_fwd / softmax_rows_bwd", "attention.hip:softmax_*_reg_kernel<16, 1> (row_blocks)", "row_blocks 8192",
         lambda d, problems, Tq, cols, ld: _softmax_reg(d, problems * Tq, ld) * 2, both(problems=37535, Tq=7, cols=9, ld=12),
         lambda d, problems, Tq, cols, ld: units(d, 3 * problems * Tq * ld)),
    Case("softmax_rows_64x2", "kernels.softmax_rows_fwd / softmax_rows_bwd", "attention.hip:softmax_*_reg_kernel<64, 2> (row_blocks)", "row_blocks 8192",
         lambda d, problems, Tq, cols, ld: _softmax_reg(d, problems * Tq, ld) * 2, both(problems=13137, Tq=5, cols=49, ld=56),
         lambda d, problems, Tq, cols, ld: units(d, 3 * problems * Tq * ld)),
    Case("softmax_rows_64x8", "kernels.softmax_rows_fwd / softmax_rows_bwd", "attention.hip:softmax_*_reg_kernel<64, 8> (row_blocks)", "row_blocks 8192",
         lambda d, problems, Tq, cols, ld: _softmax_reg(d, problems * Tq, ld) * 2, both(problems=13137, Tq=5, cols=131, ld=136),
         lambda d, problems, Tq, cols, ld: units(d, 3 * problems * Tq * ld)),
    # ---- eva.hip ---------------------------------------------------------------------------------------------------------------------
    Case("qkv_rope", "kernels.qkv_rope", "eva.hip:iseg_qkv_rope (in place)", "eva_blocks 16384",
         lambda d, B, tokens, prefix, C, hd: [lanes(B * tokens * (3 * C // 8))], only("bf16", **ROPE),      # fp32 in place: 67 M
         lambda d, B, tokens, prefix, C, hd: units(d, B * tokens * 3 * C)),
    Case("glu_fwd_scalar", "kernels.glu_fwd", "eva.hip:iseg_glu_fwd (glu_fwd_any_kernel)", "eva_blocks 16384", lambda d, rows, cols: [lanes(rows * cols)],
         both(rows=N_LANE // 5, cols=5), lambda d, rows, cols: units(d, 3 * rows * cols)),
    Case("glu_bwd_scalar", "kernels.glu_bwd", "eva.hip:iseg_glu_bwd (glu_bwd_any_kernel)", "eva_blocks 16384", lambda d, rows, cols: [lanes(rows * cols)],
         only("bf16", rows=N_LANE // 5, cols=5), lambda d, rows, cols: units(d, 5 * rows * cols)),      # fp32: 5 x 8.4 M
    # ---- dcnv3.hip ------------------------------------------------------------------------------------------------------------------
    Case("mul_colsum_vec", "kernels.mul_colsum", "dcnv3.hip:iseg_mul_colsum (mul_colsum_partial_vec_kernel, 256 of mc_blocks' 1024)", "mc_blocks -> 256",
         lambda d, rows, C: [trip(min(256, capped(cdiv(rows, 64), 1024)), 256 // min(C // 8, 256), rows)], both(rows=MC_VEC_ROWS, C=8),
         lambda d, rows, C: units(d, 2 * rows * C)),
    Case("mul_colsum_scalar", "kernels.mul_colsum", "dcnv3.hip:iseg_mul_colsum (mul_colsum_partial_kernel: contiguous row ranges of ceil(rows / grid))",
         "mc_blocks 1024", lambda d, rows, C: [trip(capped(cdiv(rows, 64), 1024), 1, rows)], both(rows=64 * 1024 + 37, C=3),
         lambda d, rows, C: units(d, 2 * rows * C)),
    Case("scale_cols_scalar", "kernels.scale_cols", "dcnv3.hip:iseg_scale_cols (scale_cols_kernel)", "lane_blocks 16384", lambda d, rows, C: [lanes(rows * C)],
         both(rows=2_796_600, C=3), lambda d, rows, C: units(d, 2 * rows * C)),
    Case("split_cols_accumulate", "kernels.split_cols_accumulate", "dcnv3.hip:iseg_split_cols_accumulate", "lane_blocks 16384",
         lambda d, rows, n0, n1, ld: [lanes(rows * (n0 + n1))], only("f32", rows=N_LANE // 5, n0=3, n1=2, ld=8),
         lambda d, rows, n0, n1, ld: rows * (ld + n0 + n1)),
    Case("dcn_mask_softmax_fwd", "kernels.dcn_mask_softmax_fwd", "dcnv3.hip:iseg_dcn_mask_softmax_fwd (in place)", "lane_blocks 16384",
         lambda d, pixels, G, P, ld: [lanes(pixels * G)], {"f32": dict(pixels=1_048_720, G=8, P=1, ld=26), "bf16": dict(pixels=2_097_440, G=4, P=2, ld=26)},
         lambda d, pixels, G, P, ld: units(d, pixels * ld)),      # fp32 with P = 2: 54.5 M
    Case("dcn_mask_softmax_bwd", "kernels.dcn_mask_softmax_bwd", "dcnv3.hip:iseg_dcn_mask_softmax_bwd (in place on the gradient)", "lane_blocks 16384",
         lambda d, pixels, G, P, ld: [lanes(pixels * G)], only("bf16", pixels=1_048_720, G=8, P=1, ld=26),      # fp32, or P = 2 in bf16: 54.5 M
         lambda d, pixels, G, P, ld: units(d, 2 * pixels * ld)),
    # ---- loss.hip / mask_loss.hip ---------------------------------------------------------------------------------------------------
    Case("softmax_ce_confusion", "kernels.softmax_ce_ignore(cm=...)", "loss.hip:iseg_softmax_ce_confusion (2048 persistent workgroups over the pixel tiles)",
         "2048 tiles", lambda d, P, C: [Trip(capped(cdiv(P, 256), 2048), capped(cdiv(P, 256), 2048), cdiv(P, 256), 1, None)],
         only("f32", P=2 * 2048 * 256 + 256 * 37 + 5, C=3), lambda d, P, C: 2 * P * C + 3 * P),
    Case("argmax_confusion", "kernels.argmax_confusion", "loss.hip:iseg_argmax_confusion", "2048 tiles",
         lambda d, P, C: [Trip(capped(cdiv(P, 256), 2048), capped(cdiv(P, 256), 2048), cdiv(P, 256), 1, None)],
         only("f32", P=2 * 2048 * 256 + 256 * 37 + 5, C=3), lambda d, P, C: P * C + 2 * P),
    Case("upsample_ce_gather", "kernels.upsample_ce", "loss.hip:iseg_upsample_ce (upsample_ce_gather_kernel)", "1024",
         lambda d, N, Hi, Wi, C, s: [trip(capped(cdiv(N * Hi * Wi * C, 256), 1024), 256, N * Hi * Wi * C)], both(N=1, Hi=420, Wi=419, C=3, s=2),
         lambda d, N, Hi, Wi, C, s: units(d, 2 * N * Hi * Wi * C, f32=N * Hi * Wi * s * s + N * (Hi + 1) * (Wi + 1) * 4 * C)),
    Case("mask_loss_px_dice", "losses.mask_loss.MaskLoss(reduction=True)", "mask_loss.hip:mask_loss_px_dice_kernel", "2048",
         lambda d, B, H, W, C: [trip(capped(cdiv(B * H * W, 256), 2048), 256, B * H * W)], only("f32", B=2, H=725, W=727, C=3),
         lambda d, B, H, W, C: B * H * W * (C + 4)),
    # ---- gemm.hip -------------------------------------------------------------------------------------------------------------------
    Case("gemm_splitk_reduce", "kernels.gemm(split_k=2, bias=...)", "gemm.hip:132 splitk_reduce_kernel", "2048",
         lambda d, M, N, K, split: [trip(capped(cdiv(M * N, 256), 2048), 256, M * N)], both(M=1030, N=1021, K=256, split=2),
         lambda d, M, N, K, split: units(d, M * K + K * N + M * N, f32=split * M * N)),
    # ---- grn.hip --------------------------------------------------------------------------------------------------------------------
    Case("grn_strips", "kernels.grn_fwd / grn_bwd", "grn.hip:grn_colsum_kernel (grn_parts strips, blockIdx.y = sample)", "grn_parts 256",
         lambda d, N, HW, C: _grn(d, N, HW, C)[:1], both(**GRN_STRIP), lambda d, N, HW, C: units(d, 4 * N * HW * C)),
    Case("grn_apply_fwd", "kernels.grn_fwd", "grn.hip:grn_apply_kernel (8192) after grn_colsum_kernel at its cap of 256", "8192 / grn_parts 256", _grn,
         only("bf16", **GRN_APPLY), lambda d, N, HW, C: units(d, 2 * N * HW * C)),      # fp32: 2 x 33.6 M; the backward apply pass: 3 x 33.6 M in bf16
    Case("grn_fold_weights", "kernels.grn_fold_weights", "grn.hip:iseg_grn_fold_weights", "4096",
         lambda d, N, Cout, C4: [trip(capped(cdiv(N * Cout * (C4 // 8), 256), 4096), 256, N * Cout * (C4 // 8))], only("bf16", N=2049, Cout=1025, C4=8),
         lambda d, N, Cout, C4: units(d, N * Cout * C4 + Cout * C4, f32=N * C4)),
    # ---- dwconv.hip / dwconv_strided.hip --------------------------------------------------------------------------------------------
    Case("dwconv_fwd_tiles", "kernels.dwconv2d (forward, and the data gradient = flip)", "dwconv.hip:launch_fwd (dwconv_fwd_kernel, 2048 / slabs)",
         "2048 / slabs", _dw_fwd, both(N=2, H=524_437, W=2, C=8, K=3, dil=16), lambda d, N, H, W, C, K, dil: units(d, 2 * N * H * W * C)),
    Case("dwconv_strided_bwd_weight", "kernels.dwconv2d_strided_bwd_weight", "dwconv_strided.hip:dws_bwd_weight_kernel (bw_partitions)", "2048 / slabs",
         lambda d, N, H, W, C, K, s: [trip(capped(min(max(2048 // cdiv(C, 32), 16), cdiv(N * cdiv(H, s) * cdiv(W, s), 8)), 1 << 30), 8, N * cdiv(H, s) * cdiv(W, s))],
         both(N=3, H=146, W=301, C=8, K=3, s=2), lambda d, N, H, W, C, K, s: units(d, N * H * W * C + N * cdiv(H, s) * cdiv(W, s) * C)),
    # ---- augment.hip / projective.hip -----------------------------------------------------------------------------------------------
    Case("normalize_image", "kernels.normalize_image", "augment.hip:iseg_normalize_image", "8192",
         lambda d, pixels: [trip(capped(cdiv(3 * pixels, 256), 8192), 256, 3 * pixels)], only("f32", pixels=1_398_200), lambda d, pixels: 6 * pixels),
    Case("augment_crop", "kernels.augment_crop_batch", "augment.hip:iseg_augment_crop_batch", "8192",
         lambda d, B, Hs, Ws, ch, cw: [trip(capped(cdiv(B * ch * cw, 256), 8192), 256, B * ch * cw)], only("f32", B=2, Hs=730, Ws=731, ch=1449, cw=1448),
         lambda d, B, Hs, Ws, ch, cw: 4 * B * Hs * Ws + 4 * B * ch * cw),
    Case("augment_channel_means", "kernels.augment_channel_means", "augment.hip:augment_means_kernel (64 workgroups per sample)", "64",
         lambda d, B, H, W: [trip(64, 256, H * W)], only("f32", B=2, H=190, W=181), lambda d, B, H, W: 3 * B * H * W),
    Case("projective_tiles", "kernels.projective_transform_batch", "projective.hip:iseg_projective_transform_batch (16384 tiles of 32 x 8 pixels)", "16384",
         lambda d, B, Hs, Ws, C: [Trip(capped(B * cdiv(Hs, 8) * cdiv(Ws, 32), 16384), capped(B * cdiv(Hs, 8) * cdiv(Ws, 32), 16384), B * cdiv(Hs, 8) * cdiv(Ws, 32), 1, None)],
         only("f32", B=2, Hs=2050, Ws=2049, C=1), lambda d, B, Hs, Ws, C: 2 * B * Hs * Ws * (C + 1)),
    # ---- defattn.hip / dcn_fixed.h --------------------------------------------------------------------------------------------------
    Case("defattn", "kernels.defattn_fwd / defattn_bwd", "defattn.hip:defattn_fwd_kernel, defattn_bwd_kernel<4>, dcn_unfix_kernel (lane_blocks)",
         "lane_blocks 16384",
         lambda d, N, H, W, heads, P, Ch: [lanes(N * H * W * heads * Ch), trip(lane_blocks(N * H * W * heads * 4), 64, N * H * W * heads),
                                           lanes(N * H * W * heads * Ch)],
         only("bf16", N=1, H=1450, W=1447, heads=1, P=1, Ch=4),      # fp32: 3 x 8.4 M + 4 x 4.2 M + the int64 accumulators; P = 2 in bf16: 42 M
         lambda d, N, H, W, heads, P, Ch: units(d, 4 * N * H * W * heads * Ch + 6 * N * H * W * heads * P, other_bytes=8 * N * H * W * heads * Ch)),
    # ---- misc.hip: the two-pass max-pool gradient ------------------------------------------------------------------------------------
    Case("pool2d_bwd_max_vec", "kernels.pool2d_bwd", "misc.hip:pool_argmax_kernel, pool_max_bwd_idx_kernel (ew_blocks)", "ew_blocks 4096",
         lambda d, N, H, W, C, k, s: [trip(misc_ew_blocks(N * H * W * C // 8), 256, N * H * W * C // 8)] * 2, only("bf16", N=1, H=1450, W=1447, C=8, k=3, s=1),
         lambda d, N, H, W, C, k, s: units(d, 3 * N * H * W * C, other_bytes=N * H * W * C)),      # fp32: 3 x 16.8 M
    Case("softmax_rows_64x32", "kernels.softmax_rows_fwd / softmax_rows_bwd (in place)", "attention.hip:softmax_*_reg_kernel<64, 32> (row_blocks)",
         "row_blocks 8192", lambda d, problems, Tq, cols, ld: _softmax_reg(d, problems * Tq, ld) * 2, only("bf16", problems=13137, Tq=5, cols=515, ld=520),
         lambda d, problems, Tq, cols, ld: units(d, 2 * problems * Tq * ld)),      # fp32: 2 x 34.2 M
    # ---- elementwise.hip: layer-scale bookkeeping (gridDim.y strips over the K rows) --------------------------------------------------
    Case("layerscale_grads", "kernels.layerscale_grads / layerscale_grads_slabs", "elementwise.hip:layerscale_stage1_kernel (64 strips x 4 rows), "
         "layerscale_slabs_kernel (128 strips x 16 rows)", "64 / 128 strips",
         lambda d, K, N, nslabs: [trip(capped(K // 32, 64), 4, K), trip(capped(K // 16, 128), 16, K)], only("f32", K=4179, N=24, nslabs=3),
         lambda d, K, N, nslabs: (nslabs + 6) * (K + 1) * N),
    Case("win_bias_table", "kernels.window_attention_table", "winattn.hip:356 win_bias_table_kernel", "4096",
         lambda d, nW, heads, T: [trip(capped(cdiv(nW * heads * 4096, 256), 4096), 256, nW * heads * 4096)], only("f32", nW=171, heads=3, T=49),
         lambda d, nW, heads, T: nW * heads * 4096 + (nW + heads) * T * T),
    # ---- dwconv.hip: the persistent kernels ------------------------------------------------------------------------------------------
    Case("dwconv_fwd_dma_rounds", "kernels.dwconv2d", "dwconv.hip:launch_fwd_dma (dwconv_fwd_dma_kernel<7, 4, 8>: 2000 units over 672 of 768 resident workgroups; "
         "the matrix-core route takes over from 2048 of its own units, 1500 here)", "768 resident workgroups",
         lambda d, N, H, W, C: [Trip(672, 672, N * cdiv(H, 8) * cdiv(W, 32) * (C // 32), 1, None)], only("bf16", N=1, H=8000, W=33, C=32),
         lambda d, N, H, W, C: units(d, 2 * N * H * W * C)),
    Case("dwconv_bwd_weight_lds", "kernels.dwconv2d_bwd_weight", "dwconv.hip:473 dwconv_bwd_weight_lds_kernel (fp32 storage, 512 / slabs workgroups)", "512 / slabs",
         lambda d, N, H, W, C: [Trip(512, 512, N * cdiv(H, min(H, 256 // 7)) * cdiv(W, 32), 1, None)], only("f32", N=3, H=20, W=11589, C=8),
         lambda d, N, H, W, C: 2 * N * H * W * C),
    # ---- Swin's window partition / reverse through the real index tables (backbones/swin.py window_index_tables) -----------------------
    Case("window_partition", "backbones.swin.window_index_tables + kernels.gather_rows", "attention.hip:iseg_gather_rows", "ew_blocks 4096",
         lambda d, N, H, W, ws, shift, C: _gather_rows(d, N * cdiv(H, ws) * ws * cdiv(W, ws) * ws, C), both(N=1, H=1450, W=1447, ws=7, shift=3, C=8),
         lambda d, N, H, W, ws, shift, C: units(d, 2 * N * cdiv(H, ws) * ws * cdiv(W, ws) * ws * C, f32=2 * N * H * W)),
    Case("window_reverse", "backbones.swin.window_index_tables + kernels.gather_rows_fma", "attention.hip:iseg_gather_rows_fma", "ew_blocks 4096",
         lambda d, N, H, W, ws, shift, C: [trip(misc_ew_blocks(N * H * W * C // 8), 256, N * H * W * C // 8)], both(N=1, H=1450, W=1447, ws=7, shift=3, C=8),
         lambda d, N, H, W, ws, shift, C: units(d, N * (cdiv(H, ws) * ws * cdiv(W, ws) * ws + H * W * (2 if d == "bf16" else 1)) * C, f32=2 * N * H * W)),
    Case("resize_bwd_x_scalar_wide", "kernels.resize_bilinear_bwd", "resize.hip:iseg_resize_bilinear_bwd (X pass, resize_bwd_axis_kernel) at a source 1171 wide",
         "cap_blocks 2048", lambda d, **s: _rs_bwd(d, cross="x", **s), only("f32", N=1, Hi=300, Wi=1171, Ho=300, Wo=2731, C=3),
         lambda d, N, Hi, Wi, Ho, Wo, C: units(d, 2 * N * Hi * Wi * C + N * Ho * Wo * C, f32=N * Ho * Wi * C)),
    # ---- sod_metrics.hip:54 ---------------------------------------------------------------------------------------------------------
    Case("sod_minmax", "kernels.sod_metrics(normalize=True)", "sod_metrics.hip:54 sod_minmax_kernel (min(256, ceil(HW / 4096)) workgroups)", "256",
         lambda d, B, H, W: [trip(capped(cdiv(H * W, 4096), 256), 256, H * W)], only("f32", B=2, H=50, W=100), lambda d, B, H, W: B * H * W),
    # ---- optim.hip ------------------------------------------------------------------------------------------------------------------
    Case("adamw_clipnorm", "optimizers.modern.AdamW(clipnorm=...)", "optim.hip:iseg_adamw_step, iseg_grad_sqnorm", "4096 x 4 blocks", _adamw,
         only("f32", total=ADAMW_N, big=OPT_BIG, count=6, clip="clipnorm"), lambda d, total, big, count, clip: 4 * total + total // 2),
    Case("sgd_global_clipnorm", "optimizers.modern.SGD(global_clipnorm=...)", "optim.hip:iseg_sgd_momentum_step, grad_sq_segments_kernel, grad_sq_total_kernel",
         "4096 x 1 block", _sgd, only("f32", total=SGD_N, big=OPT_BIG, count=601, clip="global_clipnorm"),
         lambda d, total, big, count, clip: 3 * total + total // 2),
]

BY_NAME = {c.name: c for c in CASES}


def variants():
    """(case, dtype name, shape) for every storage type of every case"""
    return [(c, d, s) for c in CASES for d, s in c.shapes.items()]
