// W4A16 (GPTQ / AWQ-repacked / compressed-tensors int4) GEMM for PREFILL-sized M at GROUP SIZE 32 on gfx950:
//   c[M, N] = a[M, K] . W,  W[k][n] = (q[k][n] - (qzero[k / 32][n] + zero_offset)) * scale[k / 32][n]
// q_weight int32 [K/8, N] in exllama order (after gptq_shuffle), qzeros int32 [K/32, N/8], scales [K/32, N] f16 | bf16.
// wna16_gemm_large.hip refuses this group size: its 64-k tile carries ONE group index and it keeps the scales / zeros of the
// whole K range resident in LDS (K = 4096 x 256 columns at group 32: 80 KiB beside the tiles).  Here:
//   * Metadata STREAMS with the weights.  A 64-k tile holds exactly two groups, so every K stage carries, next to its
//     activation rows and its 8 packed weight rows, the two scale rows and the two zero rows of the tile's columns (2.5 B per
//     16 B of weights: a stream of its own, not a table).  Each WAVE fetches the rows of its own 64 columns with two
//     4-byte direct-to-LDS loads per K tile into a wave-private 512-byte slot of the stage ([2][64] 16-bit scales,
//     [2][8] zero words): the loads ride in the same counted vmcnt window as the tile's other DMA, LDS does not grow with K,
//     and there is no table, window or extra barrier.
//   * Operands: D^T[n][m] = W^T[n][k] . A^T[k][m] with v_mfma_f32_32x32x16_f16.  One exllama dword is 8 consecutive k of one
//     column = one lane's A-operand fragment (row n = lane & 31, k = 8 (lane >> 5) .. +7 of the 16-k step) and lies in ONE
//     group; k-steps 0, 1 of a tile are its first group, 2, 3 its second.  Per K tile and (n-block, group) the lane builds
//     half2(1024 + z), half2(-64 - z) (the /16 form of the odd nibbles) and the scale pair ONCE -- 4 sets -- and every
//     dequantised fragment feeds the 4 MFMAs of the wave tile's 4 m-blocks.
//   * Numerics of wna16_gemm_large.hip: (q - z) exact through the 1024 + q trick, one f16 rounding in the multiply by the
//     group scale, fp32 accumulation, one rounding of the sum.  bf16 callers: activations widened to f16 with saturation into
//     the workspace, scales read as bf16 and converted to f16, output rounded to bf16 (RNE).
//   * Data movement: activations, packed weights, scales and zeros all go global -> LDS with direct-to-LDS loads, 3 stages,
//     loads two K tiles ahead, one raw barrier per tile.  Activations: 128-byte rows XOR-swizzled on the SOURCE address,
//     conflict-free ds_read_b128.  Weights: 8 packed rows x BN words, lane-linear, ds_read_b32 of 32 consecutive words.
//   * LDS per stage: BM x 128 B + BN x 32 B + 512 B per wave.  256 x 256 tile: 3 x (32 + 8 + 4) = 132 KiB; 256 x 128: 114;
//     128 x 256: 78; 128 x 128: 63 KiB.  The epilogue's wave-private 16 KiB transpose regions overlay the stages.
//   * Work split: workgroup = WN x WM waves, wave tile 128 rows x 64 columns, K tile 64.  XCD-aware tile order (the workgroups
//     of one XCD walk the column tiles of one activation row panel).  Small grids: K is cut into up to 16 slices of whole K
//     tiles (blockIdx.y; a slice always starts on a group boundary), every slice writes an fp32 slab and
//     wna16_g32_splitk_reduce_kernel adds the slabs in slice order -- deterministic, no flags, no atomics, nothing to reset
//     between HIP-graph replays.
#include "common.h"

namespace aphro {

typedef float g32_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* g32_lds_ptr;

constexpr int G32_GS = 32;          // the one group size this file serves
constexpr int G32_META = 512;       // bytes of one wave's scales + zeros per stage: 2 x 64 x 2 + (2 x 8 x 4, padded to 256)

struct Wna16G32Params {
  const uint16_t* a;      // [M, lda] f16
  const uint32_t* qw;     // [K/8, N] exllama order
  const uint32_t* qz;     // [K/32, N/8]
  const uint16_t* sc;     // [K/32, N] f16 (or bf16: scale_bf16)
  uint16_t* c;            // [M, N]
  int M, N, K, lda;
  int zero_offset;
  int out_bf16, scale_bf16;
  int tiles_m, tiles_n;
  int ksplit;             // > 1: blockIdx.y owns K / ksplit consecutive k and writes slab blockIdx.y of `partial`
  float* partial;         // [ksplit][M][N]
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t g32_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

__device__ __forceinline__ uint32_t g32_and_or(uint32_t a, uint32_t mask, uint32_t orv) {
  uint32_t r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(mask), "v"(orv));
  return r;
}

// a lane's constants of one (n-block, group): 1024 + z, -64 - z (the odd nibbles arrive as (1024 + 16 q) / 16), the scale
struct G32Meta { f16x2 zh, zh16, sc; };

// one exllama dword -> 8 scaled f16: ((1024 + q) - (1024 + z)) * s  (exact difference, one rounding)
__device__ __forceinline__ f16x8 g32_dequant(uint32_t w, const G32Meta& m) {
  const f16x2 inv16 = {(f16)0.0625f, (f16)0.0625f};
  const uint32_t magic = 0x64006400u;
  const uint32_t q0 = g32_and_or(w, 0x000f000fu, magic);
  const uint32_t q1 = g32_and_or(w, 0x00f000f0u, magic);
  const uint32_t w8 = w >> 8;
  const uint32_t q2 = g32_and_or(w8, 0x000f000fu, magic);
  const uint32_t q3 = g32_and_or(w8, 0x00f000f0u, magic);
  const f16x2 d0 = (__builtin_bit_cast(f16x2, q0) - m.zh) * m.sc;
  const f16x2 d1 = (__builtin_bit_cast(f16x2, q1) * inv16 + m.zh16) * m.sc;
  const f16x2 d2 = (__builtin_bit_cast(f16x2, q2) - m.zh) * m.sc;
  const f16x2 d3 = (__builtin_bit_cast(f16x2, q3) * inv16 + m.zh16) * m.sc;
  const u32x4 r = {__builtin_bit_cast(uint32_t, d0), __builtin_bit_cast(uint32_t, d1), __builtin_bit_cast(uint32_t, d2),
                   __builtin_bit_cast(uint32_t, d3)};
  return __builtin_bit_cast(f16x8, r);
}

template <int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void wna16_gemm_large_g32_kernel(Wna16G32Params p) {
  constexpr int NWAVE = WM * WN;
  constexpr int BM = 128 * WM, BN = 64 * WN, BK = 64;
  constexpr int A_STAGE = BM * BK * 2;              // bytes
  constexpr int B_STAGE = (BK / 8) * BN * 4;        // 8 packed rows
  constexpr int STAGE = A_STAGE + B_STAGE + NWAVE * G32_META;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [3][A tile | B tile | per wave: scales [2][64] 16-bit, zeros [2][8] words (+ 192 B the duplicating lanes fill)]
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
  const int G = p.K / G32_GS;
  const __amdgpu_buffer_rsrc_t ra = g32_rsrc(p.a, (uint32_t)((size_t)p.M * p.lda * 2));
  const __amdgpu_buffer_rsrc_t rb = g32_rsrc(p.qw, (uint32_t)((size_t)(p.K >> 3) * p.N * 4));
  const __amdgpu_buffer_rsrc_t rs = g32_rsrc(p.sc, (uint32_t)((size_t)G * p.N * 2));
  const __amdgpu_buffer_rsrc_t rz = g32_rsrc(p.qz, (uint32_t)((size_t)G * (p.N >> 3) * 4));

  // ---- staging (direct-to-LDS) ---------------------------------------------------------------------------------------
  // A tile: BM rows x 128 B; one DMA instruction = 8 rows (lane -> row l/8, 16-byte slot l%8).  LDS slot s' of row r holds
  // global slot s' ^ f(r), f(r) = (r >> 1) & 7.  Rows past M re-read row M - 1 (their results are never stored).
  constexpr int A_PER_WAVE = BM / 8 / NWAVE;
  int a_voff[A_PER_WAVE];
#pragma unroll
  for (int i = 0; i < A_PER_WAVE; ++i) {
    const int row = (wave * A_PER_WAVE + i) * 8 + (lane >> 3);
    const int slot = (lane & 7) ^ ((row >> 1) & 7);
    a_voff[i] = (int)(((uint32_t)min(m0 + row, p.M - 1) * (uint32_t)p.lda + (uint32_t)slot * 8u) * 2u);   // (< 4 GiB: host-checked)
  }
  // B tile: 8 packed rows x BN words; one DMA instruction = 1 KiB = 256 words, lane-linear
  constexpr int B_INSTR = B_STAGE / 1024;
  constexpr int B_PER_WAVE = B_INSTR / NWAVE;
  static_assert(B_INSTR % NWAVE == 0 && (BM / 8) % NWAVE == 0, "every wave must issue the same number of loads");
  const int b_row_bytes = p.N * 4;
  int b_voff[B_PER_WAVE];
#pragma unroll
  for (int i = 0; i < B_PER_WAVE; ++i) {
    const int d = (wave * B_PER_WAVE + i) * 256 + lane * 4;
    b_voff[i] = (n0 + d % BN) * 4 + (d / BN) * b_row_bytes;      // (row < 8: small)
  }
  // metadata of this wave's 64 columns, one 4-byte DMA instruction each (the LDS image of such a load is lane-linear):
  //   scales: lane -> group l / 32 of the tile, columns 2 (l % 32), + 1       -> 16-bit [2][64]
  //   zeros:  lane -> group (l / 8) % 2, word l % 8 (lanes 16.. repeat 0..15)  -> words [2][8]
  const int wcol0 = n0 + wn * 64;
  const int s_row_bytes = p.N * 2, z_row_bytes = (p.N >> 3) * 4;
  const int s_voff = kh * s_row_bytes + wcol0 * 2 + l31 * 4;
  const int z_voff = ((lane >> 3) & 1) * z_row_bytes + (wcol0 >> 3) * 4 + (lane & 7) * 4;
  auto stage = [&](int st, int kt) {
    unsigned char* sa = smem + st * STAGE;
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
      const int voff = a_voff[i];       // (a local copy: see wna16_gemm_large.hip on hipcc dropping the host stub otherwise)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (g32_lds_ptr)(sa + (wave * A_PER_WAVE + i) * 1024), 16, voff,
                                               (k_begin + kt * BK) * 2, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
      const int voff = b_voff[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (g32_lds_ptr)(sa + A_STAGE + (wave * B_PER_WAVE + i) * 1024), 16, voff,
                                               (int)((uint32_t)(k_begin / 8 + kt * (BK / 8)) * (uint32_t)b_row_bytes), 0, 0);
    }
    const int g0 = (k_begin + kt * BK) / G32_GS;    // first of the tile's two groups
    unsigned char* sm = sa + A_STAGE + B_STAGE + wave * G32_META;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (g32_lds_ptr)sm, 4, s_voff, (int)((uint32_t)g0 * (uint32_t)s_row_bytes), 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rz, (g32_lds_ptr)(sm + 256), 4, z_voff, g0 * z_row_bytes, 0, 0);
  };

  g32_f32x16 acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

  constexpr int DMA_PER_TILE = A_PER_WAVE + B_PER_WAVE + 2;  // per wave and K tile: the counted waits below rely on it
  stage(0, 0);
  if (ktiles > 1) stage(1, 1);

  for (int kt = 0; kt < ktiles; ++kt) {
    const int st = kt % 3;
    // tile kt has landed once at most the loads of tile kt + 1 are outstanding; a raw barrier publishes it to every wave and
    // tells everyone that stage (kt + 2) % 3 -- read during tile kt - 1 -- is free: tile kt + 2 goes out under this tile's MFMAs
    if (kt + 1 < ktiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(DMA_PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < ktiles) stage((kt + 2) % 3, kt + 2);
    const unsigned char* sa = smem + st * STAGE;
    const uint32_t* sb = reinterpret_cast<const uint32_t*>(sa + A_STAGE);
    const uint16_t* msc = reinterpret_cast<const uint16_t*>(sa + A_STAGE + B_STAGE + wave * G32_META);
    const uint32_t* mz = reinterpret_cast<const uint32_t*>(sa + A_STAGE + B_STAGE + wave * G32_META + 256);
    // the tile's two groups x the wave's two n-blocks: constants built once, used by two k-steps x 4 m-blocks each
    G32Meta meta[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int col = nb * 32 + l31;                  // column inside the wave's strip
        const uint16_t sbits = msc[h * 64 + col];
        const f16 s16 = (f16)(p.scale_bf16 ? bf16_bits_to_f32(sbits) : f16_bits_to_f32(sbits));
        const int z = (int)((mz[h * 8 + (col >> 3)] >> ((col & 7) * 4)) & 0xf) + p.zero_offset;
        const f16 a16 = __builtin_bit_cast(f16, (uint16_t)(0x6400 | z));   // 1024 + z
        const f16 b16 = (f16)(float)(-64 - z);
        meta[h][nb].sc = f16x2{s16, s16};
        meta[h][nb].zh = f16x2{a16, a16};
        meta[h][nb].zh16 = f16x2{b16, b16};
      }
    // fragments of k-step j + 1 are read from LDS while the MFMAs of step j run (two register sets)
    u32x4 af[2][4];
    uint32_t wraw[2][2];
    auto read_frags = [&](int j, u32x4 (&a4)[4], uint32_t (&w2)[2]) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) w2[nb] = sb[(2 * j + kh) * BN + wn * 64 + nb * 32 + l31];
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
      for (int nb = 0; nb < 2; ++nb) wf[nb] = g32_dequant(wraw[j & 1][nb], meta[j >> 1][nb]);   // k-steps 0, 1: group 0
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[nb], __builtin_bit_cast(f16x8, af[j & 1][mb]), acc[nb][mb], 0, 0, 0);
    }
  }
  __syncthreads();                                  // every wave is done with the stage buffers

  // ---- lane holds, for row m = mb * 32 + l31, columns nb * 32 + 8 q + 4 kh + (0..3) -----------------------------------------
  if (p.ksplit > 1) {                               // fp32 slab of this K range; summed by wna16_g32_splitk_reduce_kernel
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
__global__ void wna16_g32_splitk_reduce_kernel(const float* __restrict__ partial, uint16_t* __restrict__ c, int64_t mn, int S,
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
__global__ void wna16_g32_bf16_to_f16_rows_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int M, int K, int lda) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= (int64_t)M * K) return;
  const int row = (int)(i / K), col = (int)(i % K);
  u16x8 v = *reinterpret_cast<const u16x8*>(in + (size_t)row * lda + col);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f16_bits_sat(v[j]);
  *reinterpret_cast<u16x8*>(out + i) = v;
}

template <int WM, int WN>
static int wna16_g32_launch(const Wna16G32Params& p, hipStream_t st) {
  constexpr int BM = 128 * WM, BN = 64 * WN;
  Wna16G32Params q = p;
  q.tiles_m = (p.M + BM - 1) / BM;
  q.tiles_n = p.N / BN;
  size_t lds = 3 * ((size_t)BM * 64 * 2 + (size_t)8 * BN * 4 + (size_t)WM * WN * G32_META);
  if (lds < (size_t)WM * WN * 16384) lds = (size_t)WM * WN * 16384;   // the epilogue's wave-private transpose regions
  static bool attr_set_dev[APHRO_MAX_DEVICES] = {}; bool& attr_set = attr_set_dev[device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)wna16_gemm_large_g32_kernel<WM, WN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess) {
      set_error("wna16_gemm_large_g32: cannot raise the dynamic LDS limit");
      return APHRO_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((wna16_gemm_large_g32_kernel<WM, WN>), dim3(q.tiles_m * q.tiles_n, q.ksplit), dim3(WM * WN * 64), lds, st, q);
  APHRO_LAUNCH_CHECK();
  return APHRO_OK;
}

}  // namespace aphro

using namespace aphro;

struct Wna16G32Plan { int wm, wn, ksplit; };

// One workgroup per (tile, K slice).  256-row tiles from 129 rows up; 256-column tiles when they alone give ~200 workgroups;
// otherwise K is cut, on K-tile boundaries (= group boundaries) and no finer than 512, until ~400 two-wave (200 larger)
// workgroups exist -- as long as the fp32 slabs stay small beside the weights.
static Wna16G32Plan wna16_g32_plan(int64_t M, int64_t N, int64_t K) {
  Wna16G32Plan pl;
  pl.wm = M > 128 ? 2 : 1;
  const int64_t rows = (M + 128 * pl.wm - 1) / (128 * pl.wm);
  pl.wn = (N % 256 == 0 && rows * (N / 256) >= 200) ? 4 : 2;
  pl.ksplit = 1;
  const int64_t tiles = rows * (N / (64 * pl.wn));
  const int64_t want = pl.wm * pl.wn <= 2 ? 400 : 200;
  const int64_t slab = M * N * 4;
  for (int s = 2; s <= 16; ++s) {
    if (tiles * pl.ksplit >= want) break;
    if (K % (s * 64) == 0 && K / s >= 512 && s * slab <= (36ll << 20)) pl.ksplit = s;
  }
  return pl;
}

extern "C" int aphro_wna16_gemm_large_g32_supported(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (dtype != APHRO_F16 && dtype != APHRO_BF16) return 0;
  if (M < 1 || N < 128 || K < 64 || N % 128 != 0 || K % 64 != 0 || groups * G32_GS != K) return 0;
  const uint64_t lim = 0xffffffffull;      // every byte offset the kernel forms is 32-bit
  if ((uint64_t)M * K * 2 >= lim || (uint64_t)(K / 8) * N * 4 >= lim || (uint64_t)M * N * 2 >= lim || (uint64_t)groups * N * 2 >= lim) return 0;
  return 1;
}

extern "C" size_t aphro_wna16_gemm_large_g32_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (!aphro_wna16_gemm_large_g32_supported(M, N, K, groups, dtype)) return 0;
  const Wna16G32Plan pl = wna16_g32_plan(M, N, K);
  const size_t b = dtype == APHRO_BF16 ? ((size_t)M * K * 2 + 255) / 256 * 256 : 0;
  return b + (pl.ksplit > 1 ? (size_t)pl.ksplit * M * N * sizeof(float) : 0);
}

extern "C" int aphro_wna16_gemm_large_g32(const void* a, int64_t lda, const uint32_t* q_weight, const uint32_t* qzeros,
                                          const void* scales, void* c, void* workspace, size_t workspace_bytes, int64_t M,
                                          int64_t N, int64_t K, int64_t groups, int zero_offset, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return APHRO_OK;
  APHRO_CHECK(aphro_wna16_gemm_large_g32_supported(M, N, K, groups, dtype),
              "wna16_gemm_large_g32: M=%ld N=%ld K=%ld groups=%ld dtype=%d is not served (group size 32 exactly, N %% 128, K %% 64, operands < 4 GiB)",
              (long)M, (long)N, (long)K, (long)groups, dtype);
  APHRO_CHECK(zero_offset == 0 || zero_offset == 1, "wna16_gemm_large_g32: zero_offset must be 0 or 1 (got %d)", zero_offset);
  APHRO_CHECK(lda >= K && lda % 8 == 0 && ((uintptr_t)a % 16) == 0, "wna16_gemm_large_g32: a must be 16-byte aligned with lda %% 8 == 0, lda >= K");
  APHRO_CHECK((uint64_t)M * lda * 2 < 0xffffffffull, "wna16_gemm_large_g32: activations exceed 4 GiB");
  APHRO_CHECK(((uintptr_t)q_weight % 16) == 0 && ((uintptr_t)qzeros % 4) == 0 && ((uintptr_t)scales % 4) == 0 && ((uintptr_t)c % 16) == 0,
              "wna16_gemm_large_g32: q_weight / c must be 16-byte aligned");
  const Wna16G32Plan pl = wna16_g32_plan(M, N, K);
  const size_t need = aphro_wna16_gemm_large_g32_workspace_bytes(M, N, K, groups, dtype);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0)) {
    set_error("wna16_gemm_large_g32: workspace %zu < %zu bytes (or not 16-byte aligned)", workspace_bytes, need);
    return APHRO_ERR_WORKSPACE;
  }
  Wna16G32Params p;
  p.a = (const uint16_t*)a; p.lda = (int)lda;
  char* ws = (char*)workspace;
  if (dtype == APHRO_BF16) {
    const int64_t n8 = M * K / 8;
    hipLaunchKernelGGL(wna16_g32_bf16_to_f16_rows_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const uint16_t*)a,
                       (uint16_t*)ws, (int)M, (int)K, (int)lda);
    APHRO_LAUNCH_CHECK();
    p.a = (const uint16_t*)ws; p.lda = (int)K;
    ws += ((size_t)M * K * 2 + 255) / 256 * 256;
  }
  p.qw = q_weight; p.qz = qzeros; p.sc = (const uint16_t*)scales; p.c = (uint16_t*)c;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.zero_offset = zero_offset;
  p.out_bf16 = dtype == APHRO_BF16; p.scale_bf16 = dtype == APHRO_BF16;
  p.tiles_m = p.tiles_n = 0;
  p.ksplit = pl.ksplit; p.partial = (float*)ws;
  int rc;
  if (pl.wm == 2) rc = pl.wn == 4 ? wna16_g32_launch<2, 4>(p, st) : wna16_g32_launch<2, 2>(p, st);
  else rc = pl.wn == 4 ? wna16_g32_launch<1, 4>(p, st) : wna16_g32_launch<1, 2>(p, st);
  if (rc != APHRO_OK) return rc;
  if (pl.ksplit > 1) {
    const int64_t mn = M * N;
    hipLaunchKernelGGL(wna16_g32_splitk_reduce_kernel, dim3((unsigned)((mn / 4 + 255) / 256)), dim3(256), 0, st, p.partial,
                       (uint16_t*)c, mn, pl.ksplit, p.out_bf16);
    APHRO_LAUNCH_CHECK();
  }
  return APHRO_OK;
}
