// W8A16 (8-bit GPTQ / compressed-tensors uint8b128) GEMM for PREFILL-sized M on gfx950: c[M, N] = a[M, K] . W with
//   W[k][n] = (q[k][n] - (qzero[k / gs][n] + 1)) * scale[k / gs][n]
// on the sequential 8-bit layout (what gptq_shuffle(bit = 8) leaves and wnx_gemm.hip reads): q_weight int32 [K/4, N], word
// r of column n = k 4r .. 4r+3 (little-endian bytes); qzeros int32 [G, N/4]; scales [G, N] f16 | bf16.  Replaces
// "aphro_gptq_dequant_bits to [K, N] + library GEMM" above 64 rows (4x the packed bytes written and read per call).
//
//   * Operands: D^T[n][m] = W^T[n][k] . A^T[k][m] with v_mfma_f32_32x32x16_f16.  A lane's weight operand (row n = lane & 31,
//     k = 8 (lane >> 5) .. +7 of the 16-k step) is exactly TWO consecutive packed words (rows 2j, 2j+1) of one column, so
//     the weights never need a transposing LDS layout; a wave's read of one packed row is 128 contiguous bytes.  The
//     activations are the B operand (lane: column m = lane & 31).  One dequantised fragment feeds 4 MFMAs (4 m-blocks).
//   * int8 -> f16 in registers: two v_perm_b32 per packed word drop its bytes into the low mantissa byte of 0x6400
//     (= 1024 + q exactly, as f16 pairs); one packed subtract of 1024 + z (z = stored zero + 1 in 1..256, unmasked: the
//     difference is exact); one packed multiply by the group scale is the only rounding.  4 perm + 4 sub + 4 mul = 12 VALU
//     per 8-k fragment.  With f16 scales the MFMA operand has the bits of aphro_gptq_dequant_bits(bits = 8).
//   * bf16 callers (the rule of wna16_gemm_large.hip): activations widened to f16 with saturation into the workspace,
//     scales read as bf16 and converted to f16, fp32 accumulators, output rounded to bf16 (RNE).
//   * Data movement: activations AND weights go global -> LDS with direct-to-LDS loads (no VGPR round trip; the weight
//     tile is shared by the WM waves that own the same columns).  Activations: 128-byte rows XOR-swizzled on the SOURCE
//     address, conflict-free ds_read_b128.  Weights: the K tile's 16 packed rows, lane-linear, ds_read_b32 of 32
//     consecutive words.  3 stages: loads run two K tiles ahead, one raw barrier per tile.
//   * Group scales / zeros of the workgroup's columns are staged in LDS in WINDOWS of GWIN = 8 groups (K = 14336 at group 128
//     has 112 groups: 84 KiB for 256 columns would not fit beside three stages); crossing a window costs one extra barrier.
//   * LDS budget (largest form, 256 x 256 tile): 3 x (32 KiB activations + 16 KiB weights) + 8 x 256 x (2 + 1) B of
//     scales / zeros = 150 KiB of 160; the epilogue's 8 wave-private 16 KiB transpose regions overlay the stages.
//   * Work split: workgroup = WN x WM waves, wave tile 128 rows x 64 columns, K tile 64.  XCD-aware tile order (workgroups of
//     one XCD walk the column tiles of one activation row panel).  Small grids: K is cut into up to 16 slices of whole K
//     tiles (blockIdx.y), every slice writes an fp32 slab and gptq8_splitk_reduce_kernel adds the slabs in slice
//     order -- deterministic, no flags, no atomics, nothing to reset between HIP-graph replays.
#include "common.h"

namespace aphro {

typedef float g8_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* g8_lds_ptr;

constexpr int G8_GWIN = 8;          // quantisation groups per LDS window of scales / zeros

struct Gptq8LargeParams {
  const uint16_t* a;      // [M, lda] f16
  const uint32_t* qw;     // [K/4, N]
  const uint32_t* qz;     // [G, N/4]
  const uint16_t* sc;     // [G, N] f16 (or bf16: scale_bf16)
  uint16_t* c;            // [M, N]
  int M, N, K, lda;
  int group_size;         // multiple of 64
  int out_bf16, scale_bf16;
  int tiles_m, tiles_n;
  int ksplit;             // > 1: blockIdx.y owns K / ksplit consecutive k and writes slab blockIdx.y of `partial`
  float* partial;         // [ksplit][M][N]
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t g8_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// two packed words (8 consecutive k of one column) -> 8 scaled f16: ((1024 + q) - (1024 + z)) * s
__device__ __forceinline__ f16x8 g8_dequant(uint32_t w0, uint32_t w1, f16x2 zh, f16x2 sc) {
  const uint32_t magic = 0x64646464u;
  // v_perm_b32: selector bytes 0..3 pick from the word, 4..7 from `magic`
  const f16x2 d0 = (__builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, w0, 0x04010400u)) - zh) * sc;
  const f16x2 d1 = (__builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, w0, 0x04030402u)) - zh) * sc;
  const f16x2 d2 = (__builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, w1, 0x04010400u)) - zh) * sc;
  const f16x2 d3 = (__builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, w1, 0x04030402u)) - zh) * sc;
  const u32x4 r = {__builtin_bit_cast(uint32_t, d0), __builtin_bit_cast(uint32_t, d1), __builtin_bit_cast(uint32_t, d2),
                   __builtin_bit_cast(uint32_t, d3)};
  return __builtin_bit_cast(f16x8, r);
}

template <int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gptq8_gemm_large_kernel(Gptq8LargeParams p) {
  constexpr int NWAVE = WM * WN;
  constexpr int BM = 128 * WM, BN = 64 * WN, BK = 64;
  constexpr int A_STAGE = BM * BK * 2;              // bytes
  constexpr int B_STAGE = (BK / 4) * BN * 4;        // 16 packed rows
  constexpr int STAGE = A_STAGE + B_STAGE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [3][A tile | B tile] [scales: GWIN x BN 16-bit] [zeros: GWIN x BN/4 words]
  uint16_t* meta_sc = reinterpret_cast<uint16_t*>(smem + 3 * STAGE);
  uint32_t* meta_z = reinterpret_cast<uint32_t*>(smem + 3 * STAGE + G8_GWIN * BN * 2);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int kh = lane >> 5, l31 = lane & 31;
  // ---- this workgroup's tile and K range.  XCD x gets a contiguous range of logical tile ids; within it the column tiles
  // are the fast index (neighbours share the A row panel) ------------------------------------------------------------------
  const int ntiles = p.tiles_m * p.tiles_n;
  int tile;
  {
    const int q = ntiles / 8, r = ntiles % 8, xcd = blockIdx.x % 8, k = blockIdx.x / 8;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;      // bijective for any ntiles
  }
  const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int klen = p.K / p.ksplit, k_begin = blockIdx.y * klen;
  const int ktiles = klen / BK;
  const int g_begin = k_begin / p.group_size;
  const int G = (k_begin + klen - 1) / p.group_size - g_begin + 1;           // quantisation groups of this K range
  const __amdgpu_buffer_rsrc_t ra = g8_rsrc(p.a, (uint32_t)((size_t)p.M * p.lda * 2));
  const __amdgpu_buffer_rsrc_t rb = g8_rsrc(p.qw, (uint32_t)((size_t)(p.K >> 2) * p.N * 4));

  // groups [win, win + GWIN) of the K range -> LDS
  auto load_meta = [&](int win) {
    const int cnt = min(G8_GWIN, G - win);
    for (int i = threadIdx.x; i < cnt * (BN / 2); i += NWAVE * 64) {
      const int g = i / (BN / 2), j = i % (BN / 2);
      reinterpret_cast<uint32_t*>(meta_sc)[i] = reinterpret_cast<const uint32_t*>(p.sc)[((size_t)(g_begin + win + g) * p.N + n0) / 2 + j];
    }
    for (int i = threadIdx.x; i < cnt * (BN / 4); i += NWAVE * 64) {
      const int g = i / (BN / 4), j = i % (BN / 4);
      meta_z[i] = p.qz[(size_t)(g_begin + win + g) * (p.N >> 2) + (n0 >> 2) + j];
    }
  };
  load_meta(0);

  // ---- staging (direct-to-LDS) ---------------------------------------------------------------------------------------
  // A tile: BM rows x 128 B; one DMA instruction = 8 rows (lane -> row l/8, 16-byte slot l%8).  LDS slot s' of row r holds
  // global slot s' ^ f(r), f(r) = (r >> 1) & 7.  Rows past M re-read row M - 1 (their results are never stored).
  constexpr int A_PER_WAVE = BM / 8 / NWAVE;
  int a_voff[A_PER_WAVE];
#pragma unroll
  for (int i = 0; i < A_PER_WAVE; ++i) {
    const int row = (wave * A_PER_WAVE + i) * 8 + (lane >> 3);
    const int slot = (lane & 7) ^ ((row >> 1) & 7);
    a_voff[i] = (min(m0 + row, p.M - 1) * p.lda + slot * 8) * 2;
  }
  // B tile: 16 packed rows x BN words; one DMA instruction = 1 KiB = 256 words, lane-linear
  constexpr int B_INSTR = B_STAGE / 1024;
  constexpr int B_PER_WAVE = B_INSTR / NWAVE;
  static_assert(B_INSTR % NWAVE == 0 && (BM / 8) % NWAVE == 0, "every wave must issue the same number of loads");
  const int b_row_bytes = p.N * 4;
  int b_voff[B_PER_WAVE];
#pragma unroll
  for (int i = 0; i < B_PER_WAVE; ++i) {
    const int d = (wave * B_PER_WAVE + i) * 256 + lane * 4;
    b_voff[i] = (n0 + d % BN) * 4 + (d / BN) * b_row_bytes;
  }
  auto stage = [&](int st, int kt) {
    unsigned char* sa = smem + st * STAGE;
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
      const int voff = a_voff[i];       // (a local copy: see wna16_gemm_large.hip on hipcc dropping the host stub otherwise)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (g8_lds_ptr)(sa + (wave * A_PER_WAVE + i) * 1024), 16, voff,
                                               (k_begin + kt * BK) * 2, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
      const int voff = b_voff[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (g8_lds_ptr)(sa + A_STAGE + (wave * B_PER_WAVE + i) * 1024), 16, voff,
                                               (k_begin / 4 + kt * (BK / 4)) * b_row_bytes, 0, 0);
    }
  };

  g8_f32x16 acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

  constexpr int DMA_PER_TILE = A_PER_WAVE + B_PER_WAVE;      // per wave and K tile: the counted waits below rely on it
  stage(0, 0);
  if (ktiles > 1) stage(1, 1);
  __syncthreads();                                           // (also publishes the first window of scales / zeros)

  f16x2 zh[2], scv[2];
  int cur_group = -1, win = 0;
  for (int kt = 0; kt < ktiles; ++kt) {
    const int st = kt % 3;
    // tile kt has landed once at most the loads of tile kt + 1 are outstanding; a raw barrier publishes it to every wave and
    // tells everyone that stage (kt + 2) % 3 -- read during tile kt - 1 -- is free: tile kt + 2 goes out under this tile's MFMAs
    if (kt + 1 < ktiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(DMA_PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < ktiles) stage((kt + 2) % 3, kt + 2);
    const int grp = (k_begin + kt * BK) / p.group_size - g_begin;
    if (grp != cur_group) {                                  // workgroup-uniform: new quantisation group
      cur_group = grp;
      if (grp - win >= G8_GWIN) {
        // next window: every wave is past the barrier above, so nobody still reads the old one (it is only read here)
        win = grp;
        load_meta(win);
        __syncthreads();
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int col = wn * 64 + nb * 32 + l31;             // column inside the workgroup tile
        const uint16_t sb = meta_sc[(grp - win) * BN + col];
        const f16 s16 = (f16)(p.scale_bf16 ? bf16_bits_to_f32(sb) : f16_bits_to_f32(sb));
        const uint32_t z = ((meta_z[(grp - win) * (BN / 4) + (col >> 2)] >> ((col & 3) * 8)) & 0xffu) + 1u;   // 1..256
        const f16 z16 = __builtin_bit_cast(f16, (uint16_t)(0x6400u + z));                                   // 1024 + z
        scv[nb] = f16x2{s16, s16};
        zh[nb] = f16x2{z16, z16};
      }
    }
    const unsigned char* sa = smem + st * STAGE;
    const uint32_t* sb = reinterpret_cast<const uint32_t*>(sa + A_STAGE);
    // fragments of k-step j + 1 are read from LDS while the MFMAs of step j run (two register sets)
    u32x4 af[2][4];
    uint32_t wraw[2][2][2];
    auto read_frags = [&](int j, u32x4 (&a4)[4], uint32_t (&w2)[2][2]) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int col = wn * 64 + nb * 32 + l31;
        w2[nb][0] = sb[(4 * j + 2 * kh) * BN + col];
        w2[nb][1] = sb[(4 * j + 2 * kh + 1) * BN + col];
      }
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int row = wm * 128 + mb * 32 + l31;
        const int slot = (2 * j + kh) ^ ((row >> 1) & 7);
        a4[mb] = *reinterpret_cast<const u32x4*>(sa + row * 128 + slot * 16);
      }
    };
    read_frags(0, af[0], wraw[0]);
#pragma unroll
    for (int j = 0; j < BK / 16; ++j) {
      if (j + 1 < BK / 16) read_frags(j + 1, af[(j + 1) & 1], wraw[(j + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);            // keep the next step's LDS reads ABOVE this step's MFMAs
      f16x8 wf[2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) wf[nb] = g8_dequant(wraw[j & 1][nb][0], wraw[j & 1][nb][1], zh[nb], scv[nb]);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[nb], __builtin_bit_cast(f16x8, af[j & 1][mb]), acc[nb][mb], 0, 0, 0);
    }
  }
  __syncthreads();                                  // every wave is done with the stage buffers

  // ---- lane holds, for row m = mb * 32 + l31, columns nb * 32 + 8 q + 4 kh + (0..3) -----------------------------------------
  if (p.ksplit > 1) {                               // fp32 slab of this K range; summed by gptq8_splitk_reduce_kernel
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int row = m0 + wm * 128 + mb * 32 + l31;
      if (row >= p.M) continue;
      float* prow = p.partial + ((size_t)blockIdx.y * p.M + row) * p.N + n0 + wn * 64;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<f32x4*>(prow + nb * 32 + 8 * q + 4 * kh) =
              f32x4{acc[nb][mb][4 * q], acc[nb][mb][4 * q + 1], acc[nb][mb][4 * q + 2], acc[nb][mb][4 * q + 3]};
    }
    return;
  }
  unsigned char* region = smem + wave * 16384;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v0 = acc[nb][mb][4 * q], v1 = acc[nb][mb][4 * q + 1], v2 = acc[nb][mb][4 * q + 2], v3 = acc[nb][mb][4 * q + 3];
        epi_put(region, mb * 32 + l31, nb * 8 + 2 * q + kh,
                p.out_bf16 ? u32x2{pack2_16<true>(v0, v1), pack2_16<true>(v2, v3)} : u32x2{pack2_16<false>(v0, v1), pack2_16<false>(v2, v3)});
      }
  const int64_t origin = (int64_t)(m0 + wm * 128) * p.N + n0 + wn * 64;      // (elements); rows past M: dropped by the descriptor
  epi_flush_buf(region, p.c + origin, p.N, ((int64_t)p.M * p.N - origin) * 2, lane);
}

// partial [S][M*N] fp32 -> c [M*N] f16 / bf16 (fixed summation order: deterministic)
__global__ void gptq8_splitk_reduce_kernel(const float* __restrict__ partial, uint16_t* __restrict__ c, int64_t mn, int S,
                                           int out_bf16) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= mn) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(partial + i);
  for (int k = 1; k < S; ++k) s += *reinterpret_cast<const f32x4*>(partial + (size_t)k * mn + i);
  u16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = out_bf16 ? f32_to_bf16_bits(s[j]) : f32_to_f16_bits(s[j]);
  *reinterpret_cast<u16x4*>(c + i) = o;
}

// bf16 [M, K] (row stride lda) -> f16 [M, K] contiguous, saturating (see bf16_bits_to_f16_bits_sat)
__global__ void gptq8_bf16_to_f16_rows_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int M, int K, int lda) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= (int64_t)M * K) return;
  const int row = (int)(i / K), col = (int)(i % K);
  u16x8 v = *reinterpret_cast<const u16x8*>(in + (size_t)row * lda + col);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f16_bits_sat(v[j]);
  *reinterpret_cast<u16x8*>(out + i) = v;
}

template <int WM, int WN>
static int gptq8_launch(const Gptq8LargeParams& p, hipStream_t st) {
  constexpr int BM = 128 * WM, BN = 64 * WN;
  Gptq8LargeParams q = p;
  q.tiles_m = (p.M + BM - 1) / BM;
  q.tiles_n = p.N / BN;
  size_t lds = 3 * ((size_t)BM * 64 * 2 + (size_t)16 * BN * 4) + (size_t)G8_GWIN * BN * 3;
  if (lds < (size_t)WM * WN * 16384) lds = (size_t)WM * WN * 16384;   // the epilogue's wave-private transpose regions
  static bool attr_set_dev[APHRO_MAX_DEVICES] = {}; bool& attr_set = attr_set_dev[device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)gptq8_gemm_large_kernel<WM, WN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess) {
      set_error("gptq8_gemm_large: cannot raise the dynamic LDS limit");
      return APHRO_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((gptq8_gemm_large_kernel<WM, WN>), dim3(q.tiles_m * q.tiles_n, q.ksplit), dim3(WM * WN * 64), lds, st, q);
  APHRO_LAUNCH_CHECK();
  return APHRO_OK;
}

}  // namespace aphro

using namespace aphro;

struct Gptq8Plan { int wm, wn, ksplit; };

// One workgroup per (tile, K slice).  256-row tiles from 129 rows up; 256-column tiles when they alone give ~200 workgroups;
// otherwise K is cut, on K-tile boundaries and no finer than 512, until ~400 two-wave (200 larger) workgroups exist -- as
// long as the fp32 slabs stay small beside the weights.  A slice may begin inside a quantisation group (the kernel finds
// its groups from k): channel-wise weights (one group) are cut like any other.
static Gptq8Plan gptq8_plan(int64_t M, int64_t N, int64_t K) {
  Gptq8Plan pl;
  pl.wm = M > 128 ? 2 : 1;
  const int64_t rows = (M + 128 * pl.wm - 1) / (128 * pl.wm);
  pl.wn = (N % 256 == 0 && rows * (N / 256) >= 200) ? 4 : 2;
  { const int v = APHRO_LAB_ENV_INT("APHRO_GPTQ8_LARGE_WN", 0); if (v == 2 || (v == 4 && N % 256 == 0)) pl.wn = v; }
  pl.ksplit = 1;
  const int64_t tiles = rows * (N / (64 * pl.wn));
  const int64_t unit = 64;
  const int64_t want = pl.wm * pl.wn <= 2 ? 400 : 200;
  const int64_t slab = M * N * 4;
  for (int s = 2; s <= 16; ++s) {
    if (tiles * pl.ksplit >= want) break;
    if (K % (s * unit) == 0 && K / s >= 512 && s * slab <= (36ll << 20)) pl.ksplit = s;
  }
  { const int s = APHRO_LAB_ENV_INT("APHRO_GPTQ8_LARGE_KSPLIT", 0); if (s >= 1 && K % (s * unit) == 0) pl.ksplit = s; }
  return pl;
}

extern "C" int aphro_gptq8_gemm_large_supported(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (dtype != APHRO_F16 && dtype != APHRO_BF16) return 0;
  if (M < 1 || N < 128 || K < 64 || groups < 1 || N % 128 != 0 || K % 64 != 0 || K % groups != 0 || (K / groups) % 64 != 0) return 0;
  const uint64_t lim = 0xffffffffull;      // every byte offset the kernel forms is 32-bit
  if ((uint64_t)M * K * 2 >= lim || (uint64_t)K * N >= lim || (uint64_t)M * N * 2 >= lim || (uint64_t)groups * N * 2 >= lim) return 0;
  return 1;
}

extern "C" size_t aphro_gptq8_gemm_large_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (!aphro_gptq8_gemm_large_supported(M, N, K, groups, dtype)) return 0;
  const Gptq8Plan pl = gptq8_plan(M, N, K);
  const size_t b = dtype == APHRO_BF16 ? ((size_t)M * K * 2 + 255) / 256 * 256 : 0;
  return b + (pl.ksplit > 1 ? (size_t)pl.ksplit * M * N * sizeof(float) : 0);
}

extern "C" int aphro_gptq8_gemm_large(const void* a, int64_t lda, const uint32_t* q_weight, const uint32_t* qzeros,
                                      const void* scales, void* c, void* workspace, size_t workspace_bytes, int64_t M,
                                      int64_t N, int64_t K, int64_t groups, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return APHRO_OK;
  APHRO_CHECK(aphro_gptq8_gemm_large_supported(M, N, K, groups, dtype),
              "gptq8_gemm_large: M=%ld N=%ld K=%ld groups=%ld dtype=%d is not served (N %% 128, K %% 64, group size %% 64, operands < 4 GiB)",
              (long)M, (long)N, (long)K, (long)groups, dtype);
  APHRO_CHECK(lda >= K && lda % 8 == 0 && ((uintptr_t)a % 16) == 0, "gptq8_gemm_large: a must be 16-byte aligned with lda %% 8 == 0, lda >= K");
  APHRO_CHECK((uint64_t)M * lda * 2 < 0xffffffffull, "gptq8_gemm_large: activations exceed 4 GiB");
  APHRO_CHECK(((uintptr_t)q_weight % 16) == 0 && ((uintptr_t)qzeros % 4) == 0 && ((uintptr_t)scales % 4) == 0 && ((uintptr_t)c % 16) == 0,
              "gptq8_gemm_large: q_weight / c must be 16-byte aligned");
  const int64_t gs = K / groups;
  const Gptq8Plan pl = gptq8_plan(M, N, K);
  const size_t need = aphro_gptq8_gemm_large_workspace_bytes(M, N, K, groups, dtype);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0)) {
    set_error("gptq8_gemm_large: workspace %zu < %zu bytes (or not 16-byte aligned)", workspace_bytes, need);
    return APHRO_ERR_WORKSPACE;
  }
  Gptq8LargeParams p;
  p.a = (const uint16_t*)a; p.lda = (int)lda;
  char* ws = (char*)workspace;
  if (dtype == APHRO_BF16) {
    const int64_t n8 = M * K / 8;
    hipLaunchKernelGGL(gptq8_bf16_to_f16_rows_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const uint16_t*)a,
                       (uint16_t*)ws, (int)M, (int)K, (int)lda);
    APHRO_LAUNCH_CHECK();
    p.a = (const uint16_t*)ws; p.lda = (int)K;
    ws += ((size_t)M * K * 2 + 255) / 256 * 256;
  }
  p.qw = q_weight; p.qz = qzeros; p.sc = (const uint16_t*)scales; p.c = (uint16_t*)c;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.group_size = (int)gs;
  p.out_bf16 = dtype == APHRO_BF16; p.scale_bf16 = dtype == APHRO_BF16;
  p.tiles_m = p.tiles_n = 0;
  p.ksplit = pl.ksplit; p.partial = (float*)ws;
  int rc;
  if (pl.wm == 2) rc = pl.wn == 4 ? gptq8_launch<2, 4>(p, st) : gptq8_launch<2, 2>(p, st);
  else rc = pl.wn == 4 ? gptq8_launch<1, 4>(p, st) : gptq8_launch<1, 2>(p, st);
  if (rc != APHRO_OK) return rc;
  if (pl.ksplit > 1) {
    const int64_t mn = M * N;
    hipLaunchKernelGGL(gptq8_splitk_reduce_kernel, dim3((unsigned)((mn / 4 + 255) / 256)), dim3(256), 0, st, p.partial,
                       (uint16_t*)c, mn, pl.ksplit, p.out_bf16);
    APHRO_LAUNCH_CHECK();
  }
  return APHRO_OK;
}
