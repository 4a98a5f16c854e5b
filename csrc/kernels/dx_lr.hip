// K13: logistic-regression approximation-coefficient encoder on fp64 MFMA.
//
// One pass over the DP's raw records computes BOTH coefficient levels:
//
//   xa_i      = [1, (X_i - mean) / sd]                (standardise + augment, in registers)
//   out[a][b] = sum_i w_i * xa_i[a] * xa_i[b]          (level 2, w_i = wa*y_i + wb or w[i])
//   out[D][b] = sum_i g_i * xa_i[b],  g_i = 2 y_i - 1  (level 1, in the spare row D)
//
// Reference: lib/encoding/logistic_regression.go:61-111 computes the level-1
// and level-2 coefficients record by record through cartesian products
// (O(N (d+1)^2) scalar float ops in Go, after a separate standardisation pass,
// :367-403).  Here it is one tall-skinny GEMM over the records: K = N is the
// reduction dimension of v_mfma_f64_16x16x4f64.  For one K-step of 4 records,
// lane l holds xa[k][16t + (l&15)] (k = l>>4) for every 16-column tile t it
// works on; the same registers are the B operand and, scaled by w[k], the A
// operand.
//
// The output is cut into tile-blocks of at most 3x3 tiles (48x48): block
// (x, y, z) of a launch handles record block x and tile-block (y, z), loads the TA
// A-side and TB B-side tiles of its tile-block (the same registers on a
// diagonal tile-block) and issues TA*TB MFMAs per step.  Up to 48 rows
// (level 2 plus the level-1 row) are ONE 3x3 tile-block at offset 0, exactly
// the kernel this used to be; wider inputs take a grid of 3x3 tile-blocks
// plus narrower instantiations on the ragged right/bottom edge, so tiles that
// are entirely padding are never computed.  The level-1 vector rides in the A
// operand's spare row D (A = g_i there, B as usual) of whichever tile-block
// row holds global row D, so it costs no extra pass over HBM (it used to be a
// separate rocBLAS gemv that ran on a single workgroup).  Waves stride over
// records (grid-stride), the 4 waves of a block reduce through LDS and each
// block writes its sub-block of a PxP partial (P = 48, or the tile-padded row
// count beyond that); a tiny second pass (dx_lr_reduce: fixed summation order
// over the [blocks,P,P] slab, batched over the DPs of a rank) finishes
// deterministically.
//
// One encoder entry, dx_lr_encode, with three independent options; each only
// selects other instantiations of the one kernel template or fewer launches of
// the same ones, so a value is the same bits whichever way it is asked for:
//   upper plan (Packing = 1): level 2 is symmetric, so only (i, j), i <= j, is
//     sent.  The tile-blocks strictly below the diagonal are not launched
//     (unless they hold a level-1 row), and dx_lr_reduce_pack does block sum,
//     gather of [level 1, upper triangle] and the rounding to int64 in one launch.
//   label columns (NbrTargets = T >= 2): level 2's weight y - y (-1)^2 - 1 = -1
//     does not depend on the label, so T binary models over the same records
//     share it.  The kMulti instantiations accumulate level 1 of target t,
//     g_t = 2 Y[i][t] - 1, in row D + t: in the spare rows of the one 48-row
//     tile-block while D + T <= 48, in further row tiles beyond.
//   cells (SQL WHERE / GROUP BY): every coefficient sum is taken per cell of a
//     DP's records.  The grouped instantiations (a trailing LrCells argument)
//     read a cell's rows through a row permutation grouped by cell (made from
//     dx_group_cells' ids by a stable sort); the cells of a window are one more
//     factor of the record-block grid dimension, and the partials [cells,
//     record blocks, P, P] are finished by the reducers with the cells as items.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef double dx_f64x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kTile = 16;
constexpr int kTiles = 3;  // a tile-block is at most kTiles x kTiles tiles
constexpr int kD = kTile * kTiles;
constexpr int kWaves = 4;

struct LrArgs {
  const double *X;     // [N][dx], row stride ldx
  int64_t ldx;
  int64_t N;
  int dx;              // raw feature columns
  int aug;             // 1: prepend the constant-1 column
  const double *mean;  // [dx] or null (no standardisation)
  const double *sd;    // [dx] or null
  const double *w;     // [N] per-record level-2 weight, or null -> wa*y + wb
  const double *y;     // [N] labels (double) or null
  double wa, wb;
  int level1;          // 1: g = 2y - 1 accumulated in row D
  // multi-target encoder only (kMulti kernels): T label columns, level 1 of
  // target t in row D + t, level-2 weight the constant wb
  const double *Y;     // [N][T] labels (double), row stride ldy
  int64_t ldy;
  int T;               // level-1 rows (1 for the single-label entry points)
};

// N rows and nothing else (no augmentation, standardisation, weights, labels, level 1): an entry sets what it has
LrArgs lr_rows(const double *X, int64_t ldx, int64_t N, int dx) {
  LrArgs a{};
  a.X = X, a.ldx = ldx, a.N = N, a.dx = dx, a.T = 1;
  return a;
}

// Where one launch's tile-blocks sit in the PxP output: block (x, y, z) covers
// row tiles ta0 + TA * y .. and column tiles tb0 + TB * z .. of record block x.
struct LrGrid {
  int ta0, tb0;
  int P;  // padded output width (row stride of a partial)
};

// The grouped encoder (kCells kernels): the records of cell c0 + c are rows
// perm[cell_start[c0 + c] .. cell_start[c0 + c + 1]) of X, y and Y.  Block x of
// a launch is record block x % nbc of cell x / nbc.
struct LrCells {
  const int64_t *perm;        // [kept rows] row indices grouped by cell, record order kept inside a cell
  const int64_t *cell_start;  // [G + 1]
  int64_t c0;                 // first cell of the launch's window
  int nbc;                    // record blocks per cell
};

// kDiag: every tile-block of the launch is on the diagonal (the single 3x3
// tile-block of a narrow input): no B-side state at all.
// kMulti: T label columns (p.Y) instead of one (p.y): the A operand of row
// D + t is g_t = 2 Y[i][t] - 1, every other row is xa * wb.  The B operand,
// the K-step order, the record striding and the reductions are those of the
// single-label kernel, so each output element is the same bits as there.
// kCells: the block works on one cell's records, read through the row
// permutation (a K-step's four lanes-of-16 read four gathered rows, each still
// one contiguous read); it strides over that cell's K-steps only, a ragged
// last K-step contributes zero operands, and a block without a K-step writes
// zeros.  One cell that holds every record in order is the ungrouped kernel
// step for step.
// The grouped kernels are the instantiations with one trailing LrCells
// argument (Cells = LrCells); without it (the empty pack) the kernel, its
// signature included, is the ungrouped one.
template <int TA, int TB, bool kDiag, bool kMulti = false, class... Cells>
__global__ void __launch_bounds__(256) lr_encode_kernel(LrArgs p, double *__restrict__ partial, LrGrid g,
                                                        Cells... cells) {
  constexpr bool kCells = sizeof...(Cells) != 0;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int kk = lane >> 4;  // 0..3 record within the K-step
  const int D = p.dx + p.aug;
  const int ta = g.ta0 + TA * (int)blockIdx.y;           // first row tile
  const int tb = g.tb0 + TB * (int)blockIdx.z;           // first column tile
  const bool diag = kDiag || (TA == TB && ta == tb);     // A-side values == B-side values
  dx_f64x4 acc[TA][TB];
#pragma unroll
  for (int a = 0; a < TA; a++)
#pragma unroll
    for (int b = 0; b < TB; b++) acc[a][b] = (dx_f64x4){0.0, 0.0, 0.0, 0.0};

  // per-lane standardisation constants of the row-side and column-side columns this lane owns
  double mua[TA], sda[TA], mub[TB], sdb[TB];
  int srca[TA], srcb[TB];
#pragma unroll
  for (int t = 0; t < TA; t++) {
    const int c = (ta + t) * kTile + col;
    srca[t] = c - p.aug;  // raw column, -1 for the augmentation column
    const bool raw = (c < D) && srca[t] >= 0;
    mua[t] = (raw && p.mean) ? p.mean[srca[t]] : 0.0;
    sda[t] = (raw && p.sd) ? p.sd[srca[t]] : 1.0;
  }
  // kMulti: the label column whose level 1 this lane's row of tile t carries, or -1
  int tcol[TA];
#pragma unroll
  for (int t = 0; t < TA; t++) {
    const int c = (ta + t) * kTile + col;
    tcol[t] = (kMulti && c >= D && c < D + p.T) ? c - D : -1;
  }
#pragma unroll
  for (int t = 0; t < TB; t++) {
    const int c = (tb + t) * kTile + col;
    srcb[t] = c - p.aug;
    const bool raw = !diag && (c < D) && srcb[t] >= 0;
    mub[t] = (raw && p.mean) ? p.mean[srcb[t]] : 0.0;
    sdb[t] = (raw && p.sd) ? p.sd[srcb[t]] : 1.0;
  }

  int64_t gw = (int64_t)blockIdx.x * kWaves + wave;
  int64_t nw = (int64_t)gridDim.x * kWaves;
  int64_t steps = (p.N + 3) / 4;
  // kCells: the records are the cell's slice [first, first + count) of the permutation
  [[maybe_unused]] const int64_t *perm = nullptr;
  [[maybe_unused]] int64_t count = 0;
  if constexpr (kCells) {
    const LrCells cl = (cells, ...);
    const int64_t cell = cl.c0 + (int64_t)(blockIdx.x / (unsigned)cl.nbc);
    const int64_t first = cl.cell_start[cell];
    perm = cl.perm + first;
    count = cl.cell_start[cell + 1] - first;
    gw = (int64_t)(blockIdx.x % (unsigned)cl.nbc) * kWaves + wave;
    nw = (int64_t)cl.nbc * kWaves;
    steps = (count + 3) / 4;
  }
  for (int64_t s = gw; s < steps; s += nw) {
    int64_t row = s * 4 + kk;
    bool live;
    if constexpr (kCells) {
      live = row < count;
      row = live ? perm[row] : 0;
    } else {
      live = row < p.N;
    }
    double va[TA], vb[TB];
    double wi = 0.0, gi = 0.0;
    double ga[TA];
#pragma unroll
    for (int t = 0; t < TA; t++) ga[t] = 0.0;
    if (live) {
      if constexpr (kMulti) {
        wi = p.wb;
        const double *yr = p.Y + row * p.ldy;
#pragma unroll
        for (int t = 0; t < TA; t++)
          if (tcol[t] >= 0) ga[t] = 2.0 * yr[tcol[t]] - 1.0;
      } else {
        const double yi = p.y ? p.y[row] : 0.0;
        wi = p.w ? p.w[row] : p.wa * yi + p.wb;
        gi = 2.0 * yi - 1.0;
      }
      const double *xr = p.X + row * p.ldx;
#pragma unroll
      for (int t = 0; t < TA; t++) {
        const int c = (ta + t) * kTile + col;
        if (c >= D) va[t] = 0.0;
        else if (srca[t] < 0) va[t] = 1.0;
        else va[t] = (xr[srca[t]] - mua[t]) / sda[t];
      }
      if (!diag) {
#pragma unroll
        for (int t = 0; t < TB; t++) {
          const int c = (tb + t) * kTile + col;
          if (c >= D) vb[t] = 0.0;
          else if (srcb[t] < 0) vb[t] = 1.0;
          else vb[t] = (xr[srcb[t]] - mub[t]) / sdb[t];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < TA; t++) va[t] = 0.0;
#pragma unroll
      for (int t = 0; t < TB; t++) vb[t] = 0.0;
    }
    if (diag) {
#pragma unroll
      for (int t = 0; t < TB; t++) vb[t] = va[t < TA ? t : 0];
    }
#pragma unroll
    for (int a = 0; a < TA; a++) {
      const int c = (ta + a) * kTile + col;  // global row of the output
      const double av = kMulti ? (tcol[a] >= 0 ? ga[a] : va[a] * wi) : ((p.level1 && c == D) ? gi : va[a] * wi);
#pragma unroll
      for (int b = 0; b < TB; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, vb[b], acc[a][b], 0, 0, 0);
    }
  }

  // f64 16x16x4 C layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  constexpr int kRows = TA * kTile, kCols = TB * kTile;
  __shared__ double red[kWaves][kRows][kCols];
#pragma unroll
  for (int a = 0; a < TA; a++)
#pragma unroll
    for (int b = 0; b < TB; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) red[wave][a * kTile + kk + 4 * r][b * kTile + col] = acc[a][b][r];
  __syncthreads();
  double *out = partial + (int64_t)blockIdx.x * g.P * g.P + (int64_t)ta * kTile * g.P + tb * kTile;
  for (int e = threadIdx.x; e < kRows * kCols; e += blockDim.x) {
    const int i = e / kCols, j = e % kCols;
    out[i * g.P + j] = red[0][i][j] + red[1][i][j] + red[2][i][j] + red[3][i][j];
  }
}

// cells: the grouped kernels over n_blocks = cells of the window x record blocks per cell
template <int TA, int TB, bool kDiag = false, bool kMulti = false, bool kCells = false>
void launch_tiles(hipStream_t stream, const LrArgs &a, double *partial, int n_blocks, int ta0, int tb0, int nga,
                  int ngb, int P, const LrCells *cells = nullptr) {
  if (nga <= 0 || ngb <= 0) return;
  const LrGrid g{ta0, tb0, P};
  if constexpr (kCells)
    hipLaunchKernelGGL((lr_encode_kernel<TA, TB, kDiag, kMulti, LrCells>), dim3(n_blocks, nga, ngb), dim3(256), 0,
                       stream, a, partial, g, *cells);
  else
    hipLaunchKernelGGL((lr_encode_kernel<TA, TB, kDiag, kMulti>), dim3(n_blocks, nga, ngb), dim3(256), 0, stream, a,
                       partial, g);
}

// run-time tile-block shape (tan x tbn tiles, each 1..3; 0 = nothing to launch) -> instantiation
template <int TA, bool kMulti, bool kCells>
void launch_cols(hipStream_t stream, const LrArgs &a, double *partial, int n_blocks, int ta0, int tb0, int nga,
                 int ngb, int P, int tbn, const LrCells *cells) {
  if (tbn == 1)
    launch_tiles<TA, 1, false, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, cells);
  else if (tbn == 2)
    launch_tiles<TA, 2, false, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, cells);
  else if (tbn == 3)
    launch_tiles<TA, 3, false, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, cells);
}

template <bool kMulti, bool kCells>
void launch_rows(hipStream_t stream, const LrArgs &a, double *partial, int n_blocks, int ta0, int tb0, int nga,
                 int ngb, int P, int tan, int tbn, const LrCells *cells) {
  if (tan == 1) launch_cols<1, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, tbn, cells);
  else if (tan == 2) launch_cols<2, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, tbn, cells);
  else if (tan == 3) launch_cols<3, kMulti, kCells>(stream, a, partial, n_blocks, ta0, tb0, nga, ngb, P, tbn, cells);
}

// Padded output width: 48 while level 2 and the level-1 rows (one per label
// column) fit one 3x3 tile-block, the tile-padded row count beyond that.
int lr_padded(int D, int level1) {
  const int nt = (D + level1 + kTile - 1) / kTile;
  return nt <= kTiles ? kD : nt * kTile;
}

// Live tiles: rows 0..D+T-1 (level 2, then one level-1 row per label column),
// columns 0..D-1.  Up to 48 rows are the single diagonal 3x3 tile-block with
// the level-1 rows in its spare rows; beyond that the row tiles (ntr) and the
// column tiles (ntc <= ntr) are cut independently into full 3x3 tile-blocks
// and the ragged right column / bottom row / corner, so fb = 0 (a few columns
// under many level-1 rows) and rb = 0 with ra > 0 (level-1 rows that open a
// row tile of their own) are launches with an empty side, not special cases.
//
// upper: the plan of the packed (distinct-coefficient) layout, which reads
// level 2 only at (i, j), i <= j, and the level-1 rows D..D+T-1.  Tile-block
// (Y, Z) of the 3x3 grid lies strictly below the diagonal when Y > Z; a
// tile-block row that holds any row >= D (48 (Y + 1) > D) is launched whole,
// from column tile 0.  With one level-1 row that is the last full tile-block
// row when there is no ragged bottom row, and none otherwise.  The ragged
// bottom row holds the last live row, hence level-1 rows: always whole.  The
// ragged right column (block column fb) is on or above the diagonal for
// Y <= fb and belongs to an all-level-1 tile-block row for Y > fb (D <=
// 48 fb + 16 rb < 48 Y): always launched.
// Every launched tile-block is the same instantiation over the same record
// blocks as in the full plan, so what it writes is the same bits.
template <bool kMulti, bool kCells = false>
int launch(void *stream_, const LrArgs &a, double *partial, int n_blocks, int P, bool upper = false,
           const LrCells *cells = nullptr) {
  const int D = a.dx + a.aug;
  const int l1 = a.level1 ? a.T : 0;
  if (a.dx <= 0 || n_blocks <= 0 || a.T < 1 || a.T > 64 || P != lr_padded(D, l1)) return -2;
  if (kMulti ? (!a.Y || a.ldy < 0) : ((a.level1 || !a.w) && !a.y)) return -2;
  if (kCells != (cells != nullptr)) return -2;
  hipStream_t stream = (hipStream_t)stream_;
  if (P == kD) {
    launch_tiles<kTiles, kTiles, true, kMulti, kCells>(stream, a, partial, n_blocks, 0, 0, 1, 1, P, cells);
  } else {
    const int ntr = P / kTile, ntc = (D + kTile - 1) / kTile;
    const int fa = ntr / kTiles, ra = ntr % kTiles, fb = ntc / kTiles, rb = ntc % kTiles;
    if (!upper) {
      launch_tiles<kTiles, kTiles, false, kMulti, kCells>(stream, a, partial, n_blocks, 0, 0, fa, fb, P, cells);
    } else {
      for (int Y = 0; Y < fa; Y++) {
        const int z0 = (l1 && kD * (Y + 1) > D) ? 0 : Y;  // a tile-block row with level-1 rows: whole
        launch_tiles<kTiles, kTiles, false, kMulti, kCells>(stream, a, partial, n_blocks, Y * kTiles, z0 * kTiles, 1,
                                                            fb - z0, P, cells);
      }
    }
    launch_rows<kMulti, kCells>(stream, a, partial, n_blocks, 0, fb * kTiles, fa, 1, P, kTiles, rb, cells);
    launch_rows<kMulti, kCells>(stream, a, partial, n_blocks, fa * kTiles, 0, 1, fb, P, ra, kTiles, cells);
    launch_rows<kMulti, kCells>(stream, a, partial, n_blocks, fa * kTiles, fb * kTiles, 1, 1, P, ra, rb, cells);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "[drynx_amd native] lr_encode: %s\n", hipGetErrorString(e));
    return -1;
  }
  return 0;
}
}  // namespace

// sum_i w_i X_i X_i^T over already-prepared rows (no standardisation, no level 1).
// partial: [n_blocks][P][P], P = lr_padded(D, 0).
extern "C" int dx_lr_moments(void *stream, const double *X, const double *w, int64_t N, int D, double *partial,
                             int n_blocks, int P) {
  LrArgs a = lr_rows(X, D, N, D);
  a.w = w;
  return launch<false>(stream, a, partial, n_blocks, P);
}

// Block partials -> totals, for many encoder launches at once: out[i][e] =
// sum_b partial[i][b][e] in a fixed order (block b into accumulator b % 4,
// then combined), so a DP's coefficients are the same bits whether its
// partials are reduced alone or with the other DPs of its rank.  One thread
// per (item, element): consecutive threads read consecutive elements.
namespace {
__global__ void __launch_bounds__(256) lr_reduce_kernel(const double *__restrict__ partial, int64_t nb, int64_t n_el,
                                                        int64_t n_items, double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items * n_el) return;
  const int64_t i = t / n_el, e = t % n_el;
  const double *p = partial + i * nb * n_el + e;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int64_t b = 0;
  for (; b + 4 <= nb; b += 4) {
    s0 += p[(b + 0) * n_el];
    s1 += p[(b + 1) * n_el];
    s2 += p[(b + 2) * n_el];
    s3 += p[(b + 3) * n_el];
  }
  // block b always lands in accumulator b % 4: trailing all-zero blocks (a
  // shorter DP in a batch padded to the longest) leave the sums unchanged
  if (b < nb) s0 += p[b * n_el];
  if (b + 1 < nb) s1 += p[(b + 1) * n_el];
  if (b + 2 < nb) s2 += p[(b + 2) * n_el];
  out[t] = (s0 + s1) + (s2 + s3);
}
}  // namespace

extern "C" int dx_lr_reduce(void *stream, const double *partial, int64_t nb, int64_t n_el, int64_t n_items,
                            double *out) {
  const int64_t n = n_items * n_el;
  if (n <= 0 || nb <= 0) return -2;
  hipLaunchKernelGGL(lr_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, partial,
                     nb, n_el, n_items, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "[drynx_amd native] lr_reduce: %s\n", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Fused DP encoder: standardise + augment + level 1 + level 2 over the raw
// records X [N][dx].  partial: [n_blocks][P][P], P = lr_padded(dx + 1, T); block
// columns past the last live column tile (all padding) are not written.
// T = 1: Y is the contiguous [N] label vector (ldy is ignored), level 1 in row
// D, level-2 weight wa*y + wb.  T = 2..64: Y is [N][T] doubles with row stride
// ldy, level 1 of target t, sum_i (2 Y[i][t] - 1) xa_i, in row D + t, and ONE
// level 2 with the constant weight wb (the kMulti kernels; wa must be 0).
// upper != 0: the packed layout's launch plan: the tile-blocks strictly below
// the diagonal that hold no level-1 row are not launched, so their part of the
// slab is NOT written.  For dx_lr_reduce_pack, which never reads it.
// perm == null: n_blocks record blocks over rows 0..N-1 (cell_start, c0, nbc
// are ignored).  perm != null: the grouped kernels, the encoder per cell for
// the window [c0, c0 + cw) of a DP's G cells (wa must be 0).  perm [kept rows]
// lists the rows that belong to a cell, grouped by cell with the record order
// kept inside a cell, cell_start [G + 1] the cells' bounds in it (device
// arrays; every perm entry in [0, N), cell_start non-decreasing from 0).  Every
// cell gets nbc record blocks whatever its size (nbc comes from shapes the host
// knows, so nothing is copied back), and n_blocks is the whole grid, cw * nbc:
// a multiple of nbc.  partial: [cw][nbc][P][P], a block without records writes
// zeros.  One cell holding rows 0..N-1 in order is the ungrouped call with
// n_blocks = nbc, the same bits.
extern "C" int dx_lr_encode(void *stream, const double *X, int64_t ldx, int64_t N, int dx, const double *mean,
                            const double *sd, const double *Y, int64_t ldy, int T, double wa, double wb,
                            double *partial, int64_t n_blocks, int P, int upper, const int64_t *perm,
                            const int64_t *cell_start, int64_t c0, int nbc) {
  const bool multi = T != 1, cells = perm != nullptr;
  if (T < 1 || T > 64 || (multi && N > 1 && ldy < T) || ((multi || cells) && wa != 0.0)) return -2;
  if (n_blocks > 0x7fffffff || (cells && (!cell_start || c0 < 0 || nbc < 1 || n_blocks < nbc || n_blocks % nbc)))
    return -2;
  LrArgs a = lr_rows(X, ldx, N, dx);
  a.aug = 1, a.mean = mean, a.sd = sd, a.wa = wa, a.wb = wb, a.level1 = 1, a.T = T;
  if (multi) a.Y = Y, a.ldy = ldy;
  else a.y = Y;
  const LrCells cl{perm, cell_start, c0, nbc};
  const int nb = (int)n_blocks;
  const bool up = upper != 0;
  if (multi && cells) return launch<true, true>(stream, a, partial, nb, P, up, &cl);
  if (multi) return launch<true>(stream, a, partial, nb, P, up);
  if (cells) return launch<false, true>(stream, a, partial, nb, P, up, &cl);
  return launch<false>(stream, a, partial, nb, P, up);
}

// Block partials -> the packed integer vector a DP encrypts, in one launch:
// out[i] = [level 1 (row D, columns 0..D-1), level 2 upper triangle row-major
// (0,0),(0,1),..,(0,D-1),(1,1),..,(D-1,D-1)], entry (a, c), a <= c, at
// D + a*D - a(a-1)/2 + (c - a).  One thread per (item, packed element);
// consecutive threads read consecutive columns of a row.  The blocks are
// summed exactly as lr_reduce_kernel sums them, and the rounding is
// round_precision's fp64 operations (x = v * precision, floor(|x| + 0.5) with
// the sign of x: half away from zero, 0 for x == +-0), so a packed value is
// the same bits as the cartesian path's value at (a, c).
// T label columns (multi-target encoder): the level-1 part is T*D values,
// target t from row D + t, then the same upper triangle; T = 1 is the layout
// above.  Reads only (i, j), i <= j < D, and rows D..D+T-1, columns < D.
namespace {
__global__ void __launch_bounds__(256) lr_reduce_pack_kernel(const double *__restrict__ partial, int64_t nb, int P,
                                                             int D, int T, int64_t n_items, double precision,
                                                             int64_t *__restrict__ out, double *__restrict__ fout) {
  const int64_t n_l1 = (int64_t)T * D;
  const int64_t n_out = n_l1 + (int64_t)D * (D + 1) / 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items * n_out) return;
  const int64_t i = t / n_out, e = t % n_out;
  int64_t r, c;
  if (e < n_l1) {
    r = D + e / D;
    c = e % D;
  } else {
    const int64_t q = e - n_l1;
    // row a: the largest a with off(a) = a*D - a(a-1)/2 <= q
    const double m = 2.0 * D + 1.0;
    int64_t a = (int64_t)((m - sqrt(m * m - 8.0 * (double)q)) * 0.5);
    a = a < 0 ? 0 : (a > D - 1 ? D - 1 : a);
    while (a > 0 && a * D - a * (a - 1) / 2 > q) a--;
    while (a + 1 < D && (a + 1) * D - (a + 1) * a / 2 <= q) a++;
    r = a;
    c = a + (q - (a * D - a * (a - 1) / 2));
  }
  const int64_t n_el = (int64_t)P * P;
  const double *p = partial + i * nb * n_el + r * P + c;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int64_t b = 0;
  for (; b + 4 <= nb; b += 4) {
    s0 += p[(b + 0) * n_el];
    s1 += p[(b + 1) * n_el];
    s2 += p[(b + 2) * n_el];
    s3 += p[(b + 3) * n_el];
  }
  if (b < nb) s0 += p[b * n_el];
  if (b + 1 < nb) s1 += p[(b + 1) * n_el];
  if (b + 2 < nb) s2 += p[(b + 2) * n_el];
  const double v = (s0 + s1) + (s2 + s3);
  if (fout) fout[t] = v;
  const double x = __dmul_rn(v, precision);  // no contraction with the + 0.5 below
  const int64_t mag = (int64_t)floor(__dadd_rn(fabs(x), 0.5));
  out[t] = x > 0.0 ? mag : (x < 0.0 ? -mag : 0);
}
}  // namespace

// partial: [n_items][nb][P][P]; out: int64 [n_items][T*D + D(D+1)/2]; fout: the
// unrounded packed values (same shape, fp64) or null.
extern "C" int dx_lr_reduce_pack(void *stream, const double *partial, int64_t nb, int P, int D, int T,
                                 int64_t n_items, double precision, int64_t *out, double *fout) {
  // rows 0..D+T-1 must lie inside the slab
  if (D <= 0 || T < 1 || T > 64 || P < D + T || nb <= 0 || n_items <= 0) return -2;
  const int64_t n = n_items * ((int64_t)T * D + (int64_t)D * (D + 1) / 2);
  hipLaunchKernelGGL(lr_reduce_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     partial, nb, P, D, T, n_items, precision, out, fout);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "[drynx_amd native] lr_reduce_pack: %s\n", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Querier gradient descent for k = 2 (FindMinimumWeights, reference
// lib/encoding/logistic_regression.go:693-742; the Cost accumulation quirk and
// the "last weights with Cost >= 0" rule kept): one (d+1)x(d+1) mat-vec per
// iteration with S = A2 + A2^T, on the host.  Runs outside the Python GIL (a
// numpy loop of 450 iterations held it for ~2.6 ms beside the VN checks).
extern "C" int dx_lr_gd_k2(const double *a0, const double *S, const double *w0, int d1, double N, double lam,
                           double step, int max_iter, double C0, double C1, double C2, double *min_w) {
  std::vector<double> w(w0, w0 + d1), Sw(d1), g(d1);
  for (int i = 0; i < d1; i++) min_w[i] = w[i];
  for (int it = 0; it < max_iter; it++) {
    double wa = 0.0, wsw = 0.0, reg = 0.0;
    for (int i = 0; i < d1; i++) {
      double acc = 0.0;
      for (int j = 0; j < d1; j++) acc += S[(int64_t)i * d1 + j] * w[j];
      Sw[i] = acc;
    }
    for (int i = 0; i < d1; i++) {
      wa += w[i] * a0[i];
      wsw += w[i] * Sw[i];
      if (i) reg += w[i] * w[i];
    }
    double c = (wa * C1 + 0.5 * wsw) * C2;
    c = c / N - C0 + (lam / (2 * N)) * reg;
    if (c >= 0.0)
      for (int i = 0; i < d1; i++) min_w[i] = w[i];
    for (int i = 0; i < d1; i++) {
      g[i] = (C1 * a0[i] + C2 * Sw[i]) / N + (i ? (lam / N) * w[i] : 0.0);
      w[i] = w[i] - step * g[i];
    }
  }
  return 0;
}
