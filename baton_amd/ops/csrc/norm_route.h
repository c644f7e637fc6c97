// Host-side router of the normalization family (LayerNorm, RMSNorm,
// BatchNorm): which kernel form, grid and LDS size a call gets. Pure (no HIP,
// no torch, no environment), like gemm_plan.h and conv_route.h, so every gate
// can be checked without a GPU; the launchers in norm.hip launch exactly what
// a route names and bindings.cpp refuses from it.
#pragma once

constexpr int kNormBlock = 256;     // threads per block of every norm kernel
constexpr int kNormMaxGrid = 2048;  // row / element grids: grid-stride past it
constexpr int kNormChunk = 64;      // channels per block of a column kernel
// column kernels: blocks aimed at, and the fewest rows a block walks
constexpr int kRowColBlocks = 1024, kRowMinRows = 128;   // LayerNorm / RMSNorm
constexpr int kBnColBlocks = 2048, kBnMinRows = 64;      // BatchNorm
// BatchNorm vector passes keep 2 C (norm) / 3 C (dx) floats of per-channel
// constants in LDS: 48 KiB at either limit
constexpr int kBnNormMaxC = 6144, kBnDxMaxC = 4096;

inline int norm_vec_elems(bool bf16) { return bf16 ? 8 : 4; }   // 16 bytes

inline long long norm_ceil_div(long long a, long long b) {
  return (a + b - 1) / b;
}

// Rows of a column kernel split over grid.y: rows_per_block =
// max(min_rows, ceil(rows / max(1, blocks / chunks))).
inline void norm_col_split(long long rows, int C, int blocks, int min_rows,
                           int* chunks, int* rows_per_block, int* grid_y) {
  *chunks = (C + kNormChunk - 1) / kNormChunk;
  long long target = blocks / (*chunks > 0 ? *chunks : 1);
  if (target < 1) target = 1;
  long long rpb = norm_ceil_div(rows, target);
  if (rpb < min_rows) rpb = min_rows;
  *rows_per_block = (int)rpb;
  *grid_y = (int)norm_ceil_div(rows, rpb);
}

// LayerNorm / RMSNorm over [R, C].
struct NormRowRoute {
  // row kernels (forward, dx): one block per row, 256 threads stride the row
  bool vec;            // 16-byte vectors (C % V == 0), else element by element
  int trips;           // loop trips of a thread over the row
  int grid;            // min(R, kNormMaxGrid) blocks
  bool capped;         // R > kNormMaxGrid: blocks grid-stride over the rows
  // column kernel (dw / db): 64 channels x 4 row lanes per block
  int chunks, rows_per_block, grid_y;
  bool direct_store;   // grid_y == 1: plain stores, else fp32 atomics
};

inline NormRowRoute norm_row_route(long long R, int C, bool bf16) {
  NormRowRoute rt{};
  const int V = norm_vec_elems(bf16);
  rt.vec = (C % V) == 0;
  rt.trips = (int)norm_ceil_div(rt.vec ? C / V : C, kNormBlock);
  rt.capped = R > kNormMaxGrid;
  rt.grid = rt.capped ? kNormMaxGrid : (int)R;
  norm_col_split(R, C, kRowColBlocks, kRowMinRows, &rt.chunks,
                 &rt.rows_per_block, &rt.grid_y);
  rt.direct_store = rt.grid_y == 1;
  return rt;
}

// BatchNorm over [M, C] (NHWC flattened).
struct BnRoute {
  // stats kernels, forward and backward: always fp32 atomics
  bool stats_vec;      // 32 row lanes x 8-channel runs (C % 64 == 0), else 4 x 64
  int chunks, rows_per_block, grid_y;
  // element passes: elem_grid blocks of 256 threads, grid-strided
  bool norm_vec;       // C % V == 0 && C <= kBnNormMaxC
  bool dx_vec;         // C % V == 0 && C <= kBnDxMaxC
  bool dres_ok;        // dres is written by the vector dx pass only
  int elem_grid;       // min(kNormMaxGrid, ceil((M C / 4 + 1) / 256))
  int norm_trips, dx_trips;
  unsigned norm_lds, dx_lds;   // dynamic LDS bytes (0 for the scalar forms)
};

inline BnRoute bn_route(long long M, int C, bool bf16) {
  BnRoute rt{};
  const int V = norm_vec_elems(bf16);
  rt.stats_vec = (C % kNormChunk) == 0;
  norm_col_split(M, C, kBnColBlocks, kBnMinRows, &rt.chunks,
                 &rt.rows_per_block, &rt.grid_y);
  rt.norm_vec = (C % V) == 0 && C <= kBnNormMaxC;
  rt.dx_vec = (C % V) == 0 && C <= kBnDxMaxC;
  rt.dres_ok = rt.dx_vec;
  long long g = norm_ceil_div(M * C / 4 + 1, kNormBlock);
  if (g > kNormMaxGrid) g = kNormMaxGrid;
  if (g < 1) g = 1;
  rt.elem_grid = (int)g;
  const long long threads = g * kNormBlock;
  rt.norm_trips = (int)norm_ceil_div(rt.norm_vec ? M * C / V : M * C, threads);
  rt.dx_trips = (int)norm_ceil_div(rt.dx_vec ? M * C / V : M * C, threads);
  rt.norm_lds = rt.norm_vec ? 2u * C * (unsigned)sizeof(float) : 0u;
  rt.dx_lds = rt.dx_vec ? 3u * C * (unsigned)sizeof(float) : 0u;
  return rt;
}
