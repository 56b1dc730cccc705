// Grouped W4A16 (GPTQ / AWQ-repacked / compressed-tensors int4) GEMM for PROMPT-sized mixture-of-experts batches on gfx950:
//   out[r, :] = A[row(r), :] . W_e,   e = expert_ids[r / 128],   W_e[k][n] = (q_e[k][n] - (z_e[k / gs][n] + zero_offset)) * s_e[k / gs][n]
// over the rows r of moe_align_block_size(topk_ids, 128, E): q_weight int32 [E, K/8, N] in exllama order, qzeros int32
// [E, G, N/8], scales [E, G, N] f16 | bf16 (the layouts of Wna16Experts), group size gs = 128 x 2^n.
// The decode-sized grouped kernel (wna16_gemm.hip) gives every 16 routed rows a workgroup that streams and dequantises the
// expert's whole column range: at ~2048 rows per expert that is 128 passes over the same weights behind a fragment-major
// gather pass.  This file is a tile machine of its own:
//   * Row tile = 128 rows of ONE expert (the alignment block), column tile BN = 128 (2 waves) or 256 (4 waves), K tile 64;
//     wave tile 128 rows x 64 columns.  A workgroup reads num_tokens_post_pad and expert_ids[tile] once and leaves when its
//     tile lies past the padded count or carries no expert: the grid is the host-side upper bound T topk + E 127 rounded up,
//     nothing synchronises with the host, the launch replays under a HIP graph with any routing of the same T.
//   * The gather is part of the loader.  Tile row r reads A row sorted_token_ids[r] / topk (GEMM 1; a null sorted_token_ids
//     is the identity: GEMM 2 reads its input in sorted order): that row's byte offset is the per-lane source offset of the
//     direct-to-LDS activation loads, computed once per workgroup.  Padding rows (sorted id = T topk) clamp to the last row
//     of A; their results are written and never consumed.  No gathered or fragment-major copy of the activations exists.
//   * Operands: D^T[n][m] = W^T[n][k] . A^T[k][m] with v_mfma_f32_32x32x16_f16.  One exllama dword is 8 consecutive k of one
//     column = one lane's A-operand fragment (row n = lane & 31, k = 8 (lane >> 5) .. +7 of the 16-k step); every dequantised
//     fragment feeds the 4 MFMAs of the wave tile's 4 m-blocks.
//   * Scales and zeros: a K tile lies in one group.  Each wave's 64 scales and 8 zero words of the tile's group ride with
//     the tile as two 4-byte direct-to-LDS loads into a wave-private 512-byte slot (constant load count per tile: one
//     counted vmcnt window, no table that grows with K), and the lane rebuilds half2(1024 + z), half2(-64 - z) and the scale
//     pair only at a group's first K tile -- once per group, i.e. every 2 x 2^n tiles.
//   * Numerics of wna16_gemm_large.hip: (q - z) exact through the 1024 + q trick, one f16 rounding in the multiply by the
//     group scale, fp32 accumulation, one rounding of the sum.  bf16 callers: the un-gathered activations are widened to f16
//     with saturation once per call into the workspace, scales read as bf16, output rounded to bf16 (RNE).
//   * Data movement: activations, packed weights and metadata go global -> LDS with direct-to-LDS loads, 3 stages, loads two
//     K tiles ahead, one raw barrier per tile.  Activations: 128-byte rows XOR-swizzled on the SOURCE address, conflict-free
//     ds_read_b128.  Weights: 8 packed rows x BN words, lane-linear, ds_read_b32 of 32 consecutive words.
//   * LDS per stage: 128 x 128 B + BN x 32 B + 512 B per wave.  BN = 128: 3 x (16 + 4 + 1) = 63 KiB; BN = 256: 3 x (16 + 8 + 2)
//     = 78 KiB.  The kernel holds one wave per SIMD (128 accumulator + ~200 other registers), i.e. two 2-wave or one 4-wave
//     workgroup per CU.  The epilogue's wave-private 16 KiB transpose regions overlay the stages.
//   * Tile order: XCD-aware.  XCD x gets a contiguous range of logical tiles with the column tile as the fast index, so
//     the workgroups of one XCD walk the column tiles of one row tile: the gathered activation panel and the expert's weight
//     columns are reused from that XCD's L2.
//   * Epilogues.  out: [m_pad, N] in the scales' dtype through the LDS transpose.  silu (GEMM 1 over the interleaved
//     (gate_j, up_j) columns of Wna16Experts.w13): act [m_pad, N / 2] row-major F16 in the arithmetic of wna16_gemm_large_silu
//     -- round(round(silu(round(gate))) * round(up)) in the scales' dtype; a bf16 result is then stored as f16 (saturating:
//     every finite bf16 within range is exact in f16) so that GEMM 2 reads f16 without a widening pass.  slab (GEMM 2): one
//     fp32 slab [1, m_pad, N] for moe_combine, which applies the routed weight, rounds and sums the top-k rows in slot order.
//   * No split-K (prompt-sized batches fill the chip with row tiles), no act-order, no FP8 experts.
#include "common.h"

namespace aphro {

typedef float moel_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* moel_lds_ptr;

constexpr int MOEL_BM = 128;         // rows of a tile = the block size of moe_align_block_size
constexpr int MOEL_META = 512;       // bytes of one wave's scales + zeros per stage: 64 x 2 (+ the duplicating lanes) + 8 x 4 (padded)
enum { MOEL_OUT = 0, MOEL_SILU = 1, MOEL_SLAB = 2 };

struct MoeLargeParams {
  const uint16_t* a;            // [a_rows, lda] f16
  const int32_t* sorted;        // [>= post_pad] slot ids in expert order (row = id / topk), or null: identity
  const int32_t* expert_ids;    // [m_pad / 128]
  const int32_t* post_pad;      // [1]
  const uint32_t* qw;           // [E, K/8, N] exllama order
  const uint32_t* qz;           // [E, G, N/8]
  const uint16_t* sc;           // [E, G, N] f16 (or bf16: scale_bf16)
  void* c;                      // out: 16-bit [m_pad, N]; silu: f16 [m_pad, N/2]; slab: fp32 [m_pad, N]
  int a_rows, lda, topk;
  int row_limit;                // rows that may be touched: min(m_pad, length of sorted)
  int m_pad, N, K, groups;
  int gs_tiles;                 // K tiles per group (a power of two >= 2)
  int num_experts, zero_offset;
  int out_bf16, scale_bf16, mode;
  int tiles_m, tiles_n;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t moel_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

__device__ __forceinline__ uint32_t moel_and_or(uint32_t a, uint32_t mask, uint32_t orv) {
  uint32_t r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(mask), "v"(orv));
  return r;
}

// a lane's constants of one (n-block, group): 1024 + z, -64 - z (the odd nibbles arrive as (1024 + 16 q) / 16), the scale
struct MoelMeta { f16x2 zh, zh16, sc; };

// one exllama dword -> 8 scaled f16: ((1024 + q) - (1024 + z)) * s  (exact difference, one rounding)
__device__ __forceinline__ f16x8 moel_dequant(uint32_t w, const MoelMeta& m) {
  const f16x2 inv16 = {(f16)0.0625f, (f16)0.0625f};
  const uint32_t magic = 0x64006400u;
  const uint32_t q0 = moel_and_or(w, 0x000f000fu, magic);
  const uint32_t q1 = moel_and_or(w, 0x00f000f0u, magic);
  const uint32_t w8 = w >> 8;
  const uint32_t q2 = moel_and_or(w8, 0x000f000fu, magic);
  const uint32_t q3 = moel_and_or(w8, 0x00f000f0u, magic);
  const f16x2 d0 = (__builtin_bit_cast(f16x2, q0) - m.zh) * m.sc;
  const f16x2 d1 = (__builtin_bit_cast(f16x2, q1) * inv16 + m.zh16) * m.sc;
  const f16x2 d2 = (__builtin_bit_cast(f16x2, q2) - m.zh) * m.sc;
  const f16x2 d3 = (__builtin_bit_cast(f16x2, q3) * inv16 + m.zh16) * m.sc;
  const u32x4 r = {__builtin_bit_cast(uint32_t, d0), __builtin_bit_cast(uint32_t, d1), __builtin_bit_cast(uint32_t, d2),
                   __builtin_bit_cast(uint32_t, d3)};
  return __builtin_bit_cast(f16x8, r);
}

// two (gate, up) pairs -> two activations, one dword of F16 (see the file header on bf16)
template <typename T>
__device__ __forceinline__ uint32_t moel_silu2(float g0, float u0, float g1, float u1) {
  uint16_t a0 = silu_mul_bits<T>(T::to_f32(T::from_f32(g0)), T::to_f32(T::from_f32(u0)));
  uint16_t a1 = silu_mul_bits<T>(T::to_f32(T::from_f32(g1)), T::to_f32(T::from_f32(u1)));
  if constexpr (!__is_same(T, Half)) {
    a0 = bf16_bits_to_f16_bits_sat(a0);
    a1 = bf16_bits_to_f16_bits_sat(a1);
  }
  return (uint32_t)a0 | ((uint32_t)a1 << 16);
}

template <int WN>
__global__ __launch_bounds__(WN * 64) void moe_wna16_gemm_large_kernel(MoeLargeParams p) {
  constexpr int NWAVE = WN;
  constexpr int BM = MOEL_BM, BN = 64 * WN, BK = 64;
  constexpr int A_STAGE = BM * BK * 2;              // bytes
  constexpr int B_STAGE = (BK / 8) * BN * 4;        // 8 packed rows
  constexpr int STAGE = A_STAGE + B_STAGE + NWAVE * MOEL_META;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [3][A tile | B tile | per wave: scales [64] 16-bit (+ 128 B the duplicating lanes fill), zeros [8] words (+ 224 B likewise)]
  const int lane = threadIdx.x & 63;
  const int wn = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave = its 64-column strip
  const int kh = lane >> 5, l31 = lane & 31;
  // ---- this workgroup's tile.  XCD x gets a contiguous range of logical tile ids; within it the column tiles are the fast
  // index (neighbours share the gathered A panel and the expert) -----------------------------------------------------------
  const int ntiles = p.tiles_m * p.tiles_n;
  int tile;
  {
    const int q = ntiles / 8, r = ntiles % 8, xcd = blockIdx.x % 8, k = blockIdx.x / 8;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;      // bijective for any ntiles
  }
  const int tm = tile / p.tiles_n, tn = tile % p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  // ---- tile skipping: past the padded count, or no expert (both uniform: the whole workgroup leaves before any barrier) ----
  if (m0 + BM > min(p.post_pad[0], p.row_limit)) return;
  const int e = p.expert_ids[tm];
  if (e < 0 || e >= p.num_experts) return;
  const int ktiles = p.K / BK;
  const size_t qw_bytes = (size_t)(p.K >> 3) * p.N * 4, sc_bytes = (size_t)p.groups * p.N * 2, qz_bytes = (size_t)p.groups * (p.N >> 3) * 4;
  const __amdgpu_buffer_rsrc_t ra = moel_rsrc(p.a, (uint32_t)((size_t)p.a_rows * p.lda * 2));
  const __amdgpu_buffer_rsrc_t rb = moel_rsrc(reinterpret_cast<const char*>(p.qw) + (size_t)e * qw_bytes, (uint32_t)qw_bytes);
  const __amdgpu_buffer_rsrc_t rs = moel_rsrc(reinterpret_cast<const char*>(p.sc) + (size_t)e * sc_bytes, (uint32_t)sc_bytes);
  const __amdgpu_buffer_rsrc_t rz = moel_rsrc(reinterpret_cast<const char*>(p.qz) + (size_t)e * qz_bytes, (uint32_t)qz_bytes);

  // ---- staging (direct-to-LDS) ---------------------------------------------------------------------------------------
  // A tile: 128 rows x 128 B; one DMA instruction = 8 rows (lane -> row l/8, 16-byte slot l%8).  LDS slot s' of row r holds
  // global slot s' ^ f(r), f(r) = (r >> 1) & 7.  THE GATHER: the source row of tile row r is sorted[m0 + r] / topk, clamped
  // into A (padding ids point one row past it; a corrupt id cannot leave the buffer either).
  constexpr int A_PER_WAVE = BM / 8 / NWAVE;
  int a_voff[A_PER_WAVE];
#pragma unroll
  for (int i = 0; i < A_PER_WAVE; ++i) {
    const int row = (wn * A_PER_WAVE + i) * 8 + (lane >> 3);
    const int slot = (lane & 7) ^ ((row >> 1) & 7);
    uint32_t src = (uint32_t)(m0 + row);
    if (p.sorted) src = (uint32_t)p.sorted[m0 + row] / (uint32_t)p.topk;
    src = min(src, (uint32_t)(p.a_rows - 1));
    a_voff[i] = (int)((src * (uint32_t)p.lda + (uint32_t)slot * 8u) * 2u);   // (< 4 GiB: host-checked)
  }
  // B tile: 8 packed rows x BN words; one DMA instruction = 1 KiB = 256 words, lane-linear
  constexpr int B_INSTR = B_STAGE / 1024;
  constexpr int B_PER_WAVE = B_INSTR / NWAVE;
  static_assert(B_INSTR % NWAVE == 0 && (BM / 8) % NWAVE == 0, "every wave must issue the same number of loads");
  const int b_row_bytes = p.N * 4;
  int b_voff[B_PER_WAVE];
#pragma unroll
  for (int i = 0; i < B_PER_WAVE; ++i) {
    const int d = (wn * B_PER_WAVE + i) * 256 + lane * 4;
    b_voff[i] = (n0 + d % BN) * 4 + (d / BN) * b_row_bytes;      // (row < 8: small)
  }
  // metadata of this wave's 64 columns in the tile's group, one 4-byte DMA instruction each (lane-linear LDS image):
  //   scales: lane -> columns 2 (l % 32), + 1 (lanes 32.. repeat)   zeros: lane -> word l % 8 (lanes 8.. repeat)
  const int wcol0 = n0 + wn * 64;
  const int s_row_bytes = p.N * 2, z_row_bytes = (p.N >> 3) * 4;
  const int s_voff = wcol0 * 2 + l31 * 4;
  const int z_voff = (wcol0 >> 3) * 4 + (lane & 7) * 4;
  const int gs_shift = __builtin_ctz(p.gs_tiles);
  auto stage = [&](int st, int kt) {
    unsigned char* sa = smem + st * STAGE;
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
      const int voff = a_voff[i];       // (a local copy: see wna16_gemm_large.hip on hipcc dropping the host stub otherwise)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (moel_lds_ptr)(sa + (wn * A_PER_WAVE + i) * 1024), 16, voff, kt * BK * 2, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
      const int voff = b_voff[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (moel_lds_ptr)(sa + A_STAGE + (wn * B_PER_WAVE + i) * 1024), 16, voff,
                                               (int)((uint32_t)(kt * (BK / 8)) * (uint32_t)b_row_bytes), 0, 0);
    }
    const int g = kt >> gs_shift;
    unsigned char* sm = sa + A_STAGE + B_STAGE + wn * MOEL_META;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (moel_lds_ptr)sm, 4, s_voff, (int)((uint32_t)g * (uint32_t)s_row_bytes), 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rz, (moel_lds_ptr)(sm + 256), 4, z_voff, g * z_row_bytes, 0, 0);
  };

  moel_f32x16 acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

  constexpr int DMA_PER_TILE = A_PER_WAVE + B_PER_WAVE + 2;  // per wave and K tile: the counted waits below rely on it
  stage(0, 0);
  if (ktiles > 1) stage(1, 1);

  MoelMeta meta[2];                                 // the current group's constants of the wave's two n-blocks
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
    if ((kt & (p.gs_tiles - 1)) == 0) {             // first K tile of a group: rebuild the constants (once per group)
      const uint16_t* msc = reinterpret_cast<const uint16_t*>(sa + A_STAGE + B_STAGE + wn * MOEL_META);
      const uint32_t* mz = reinterpret_cast<const uint32_t*>(sa + A_STAGE + B_STAGE + wn * MOEL_META + 256);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int col = nb * 32 + l31;              // column inside the wave's strip
        const uint16_t sbits = msc[col];
        const f16 s16 = (f16)(p.scale_bf16 ? bf16_bits_to_f32(sbits) : f16_bits_to_f32(sbits));
        const int z = (int)((mz[col >> 3] >> ((col & 7) * 4)) & 0xf) + p.zero_offset;
        const f16 a16 = __builtin_bit_cast(f16, (uint16_t)(0x6400 | z));   // 1024 + z
        const f16 b16 = (f16)(float)(-64 - z);
        meta[nb].sc = f16x2{s16, s16};
        meta[nb].zh = f16x2{a16, a16};
        meta[nb].zh16 = f16x2{b16, b16};
      }
    }
    // fragments of k-step j + 1 are read from LDS while the MFMAs of step j run (two register sets)
    u32x4 af[2][4];
    uint32_t wraw[2][2];
    auto read_frags = [&](int j, u32x4 (&a4)[4], uint32_t (&w2)[2]) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) w2[nb] = sb[(2 * j + kh) * BN + wn * 64 + nb * 32 + l31];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int row = mb * 32 + l31;
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
      for (int nb = 0; nb < 2; ++nb) wf[nb] = moel_dequant(wraw[j & 1][nb], meta[nb]);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[nb], __builtin_bit_cast(f16x8, af[j & 1][mb]), acc[nb][mb], 0, 0, 0);
    }
  }
  __syncthreads();                                  // every wave is done with the stage buffers

  // ---- lane holds, for row m = mb * 32 + l31, columns nb * 32 + 8 q + 4 kh + (0..3); every row of an active tile is < m_pad ----
  if (p.mode == MOEL_SLAB) {                        // GEMM 2: fp32, for moe_combine (routed weight, rounding, top-k sum)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      float* prow = reinterpret_cast<float*>(p.c) + (size_t)(m0 + mb * 32 + l31) * p.N + n0 + wn * 64;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<f32x4*>(prow + nb * 32 + 8 * q + 4 * kh) =
              f32x4{acc[nb][mb][4 * q], acc[nb][mb][4 * q + 1], acc[nb][mb][4 * q + 2], acc[nb][mb][4 * q + 3]};
    }
    return;
  }
  unsigned char* region = smem + wn * 16384;
  if (p.mode == MOEL_SILU) {
    // a lane's 4 consecutive columns of an accumulator quad are two (gate, up) pairs -> two activations = one dword.  The wave
    // tile becomes 128 rows x 32 activations: a [128][64 B] image in the wave's LDS region, the 16-byte chunk XOR-ed with
    // (row >> 2) & 3, flushed as whole 64-byte row segments (the layout of wna16_gemm_large.hip's SiluAndMul epilogue).
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = mb * 32 + l31, c4 = nb * 8 + 2 * q + kh;           // 4-byte chunk 0..15 of the row
          const float v0 = acc[nb][mb][4 * q], v1 = acc[nb][mb][4 * q + 1], v2 = acc[nb][mb][4 * q + 2], v3 = acc[nb][mb][4 * q + 3];
          const uint32_t w2 = p.out_bf16 ? moel_silu2<BFloat>(v0, v1, v2, v3) : moel_silu2<Half>(v0, v1, v2, v3);
          *reinterpret_cast<uint32_t*>(region + row * 64 + ((((c4 >> 2) ^ ((row >> 2) & 3)) << 4) | ((c4 & 3) << 2))) = w2;
        }
    const int64_t ldc = p.N / 2;
    uint16_t* cs = reinterpret_cast<uint16_t*>(p.c);
    const int64_t origin = (int64_t)m0 * ldc + (n0 + wn * 64) / 2;      // (elements of the activation)
    const int64_t bytes_left = ((int64_t)p.m_pad * ldc - origin) * 2;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
        cs + origin, 0, (uint32_t)(bytes_left > 0xffffffffll ? 0xffffffffll : (bytes_left < 0 ? 0 : bytes_left)), 0x00020000);
    const int r16 = lane >> 2, c16 = lane & 3;
    u32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = i * 16 + r16;
      v[i] = *reinterpret_cast<const u32x4*>(region + row * 64 + ((c16 ^ ((row >> 2) & 3)) << 4));
    }
    const uint32_t voff = (uint32_t)r16 * (uint32_t)ldc * 2u + (uint32_t)c16 * 16u;
#pragma unroll
    for (int i = 0; i < 8; ++i) __builtin_amdgcn_raw_buffer_store_b128(v[i], rc, voff, (uint32_t)i * 16u * (uint32_t)ldc * 2u, 0);
    return;
  }
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
  const int64_t origin = (int64_t)m0 * p.N + n0 + wn * 64;      // (elements)
  epi_flush_buf(region, reinterpret_cast<uint16_t*>(p.c) + origin, p.N, ((int64_t)p.m_pad * p.N - origin) * 2, lane);
}

// bf16 [M, K] (row stride lda) -> f16 [M, K] contiguous, saturating (see bf16_bits_to_f16_bits_sat)
__global__ void moe_wna16_large_bf16_to_f16_rows_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int M, int K, int lda) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= (int64_t)M * K) return;
  const int row = (int)(i / K), col = (int)(i % K);
  u16x8 v = *reinterpret_cast<const u16x8*>(in + (size_t)row * lda + col);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f16_bits_sat(v[j]);
  *reinterpret_cast<u16x8*>(out + i) = v;
}

template <int WN>
static int moe_wna16_large_launch(const MoeLargeParams& p, hipStream_t st) {
  constexpr int BN = 64 * WN;
  MoeLargeParams q = p;
  q.tiles_m = p.m_pad / MOEL_BM;
  q.tiles_n = p.N / BN;
  size_t lds = 3 * ((size_t)MOEL_BM * 64 * 2 + (size_t)8 * BN * 4 + (size_t)WN * MOEL_META);
  if (lds < (size_t)WN * 16384) lds = (size_t)WN * 16384;   // the epilogue's wave-private transpose regions
  static bool attr_set_dev[APHRO_MAX_DEVICES] = {}; bool& attr_set = attr_set_dev[device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)moe_wna16_gemm_large_kernel<WN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess) {
      set_error("moe_wna16_gemm_large: cannot raise the dynamic LDS limit");
      return APHRO_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((moe_wna16_gemm_large_kernel<WN>), dim3(q.tiles_m * q.tiles_n), dim3(WN * 64), lds, st, q);
  APHRO_LAUNCH_CHECK();
  return APHRO_OK;
}

}  // namespace aphro

using namespace aphro;

// 256-column tiles (4 waves sharing one A tile: half the activation traffic per weight column) once they alone are two rounds
// of one workgroup per CU at the upper-bound row-tile count; 128-column tiles below that, where workgroup count matters more.
static int moe_wna16_large_bn(int64_t m_pad, int64_t N) {
  return (N % 256 == 0 && (m_pad / MOEL_BM) * (N / 256) >= 2 * (int64_t)device_cu_count()) ? 256 : 128;
}

extern "C" int aphro_moe_wna16_gemm_large_supported(int64_t m_pad, int64_t N, int64_t K, int64_t groups, int64_t num_experts,
                                                    int dtype) {
  if (dtype != APHRO_F16 && dtype != APHRO_BF16) return 0;
  if (m_pad < MOEL_BM || m_pad % MOEL_BM != 0 || N < 128 || N % 128 != 0 || K < 128 || K % 128 != 0 || groups < 1 || num_experts < 1) return 0;
  if (K % groups != 0) return 0;
  const int64_t gs = K / groups;
  if (gs % 128 != 0 || ((gs / 128) & (gs / 128 - 1)) != 0) return 0;       // 128 x 2^n: a K tile lies in one group
  const uint64_t lim = 0xffffffffull;      // every byte offset the kernel forms inside one expert / the outputs is 32-bit
  if ((uint64_t)(K / 8) * N * 4 >= lim || (uint64_t)groups * N * 2 >= lim || (uint64_t)m_pad * N * 4 >= lim || (uint64_t)m_pad * K * 2 >= lim) return 0;
  return 1;
}

extern "C" size_t aphro_moe_wna16_gemm_large_workspace_bytes(int64_t a_rows, int64_t K, int a_dtype) {
  if (a_dtype != APHRO_BF16 || a_rows < 1 || K < 1) return 0;
  return ((size_t)a_rows * K * 2 + 255) / 256 * 256;
}

extern "C" int aphro_moe_wna16_gemm_large(const void* a, int64_t a_rows, int64_t lda, int a_dtype, const int32_t* sorted_token_ids,
                                          int64_t sorted_len, int topk, const uint32_t* q_weight, const uint32_t* qzeros,
                                          const void* scales, const int32_t* expert_ids, const int32_t* num_tokens_post_pad,
                                          void* out, void* workspace, size_t workspace_bytes, int64_t m_pad, int64_t N, int64_t K,
                                          int64_t groups, int64_t num_experts, int zero_offset, int dtype, int mode, int bn,
                                          void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APHRO_CHECK(aphro_moe_wna16_gemm_large_supported(m_pad, N, K, groups, num_experts, dtype),
              "moe_wna16_gemm_large: m_pad=%ld N=%ld K=%ld groups=%ld experts=%ld dtype=%d is not served (m_pad %% 128, N %% 128, "
              "K %% 128, group size 128 x 2^n, operands < 4 GiB)", (long)m_pad, (long)N, (long)K, (long)groups, (long)num_experts, dtype);
  APHRO_CHECK(mode == MOEL_OUT || mode == MOEL_SILU || mode == MOEL_SLAB, "moe_wna16_gemm_large: mode must be 0 (out), 1 (silu) or 2 (slab), got %d", mode);
  APHRO_CHECK(bn == 0 || bn == 128 || (bn == 256 && N % 256 == 0), "moe_wna16_gemm_large: bn must be 0 (planned), 128 or 256 with N %% 256 == 0 (got %d)", bn);
  APHRO_CHECK(a_dtype == APHRO_F16 || a_dtype == APHRO_BF16, "moe_wna16_gemm_large: activations must be f16 or bf16");
  APHRO_CHECK(zero_offset == 0 || zero_offset == 1, "moe_wna16_gemm_large: zero_offset must be 0 or 1 (got %d)", zero_offset);
  APHRO_CHECK(a && q_weight && qzeros && scales && expert_ids && num_tokens_post_pad && out, "moe_wna16_gemm_large: null operand");
  APHRO_CHECK(a_rows >= 1 && lda >= K && lda % 8 == 0 && ((uintptr_t)a % 16) == 0,
              "moe_wna16_gemm_large: a must be 16-byte aligned with a_rows >= 1, lda %% 8 == 0, lda >= K");
  APHRO_CHECK((uint64_t)a_rows * lda * 2 < 0xffffffffull, "moe_wna16_gemm_large: activations exceed 4 GiB");
  if (sorted_token_ids) {
    APHRO_CHECK(topk >= 1 && sorted_len >= MOEL_BM, "moe_wna16_gemm_large: sorted_token_ids needs topk >= 1 and at least one 128-row tile (topk=%d, len=%ld)",
                topk, (long)sorted_len);
  } else {
    APHRO_CHECK(a_rows >= m_pad, "moe_wna16_gemm_large: without sorted_token_ids a holds the m_pad rows themselves (a_rows=%ld < %ld)",
                (long)a_rows, (long)m_pad);
  }
  APHRO_CHECK(((uintptr_t)q_weight % 16) == 0 && ((uintptr_t)qzeros % 4) == 0 && ((uintptr_t)scales % 4) == 0 && ((uintptr_t)out % 16) == 0,
              "moe_wna16_gemm_large: q_weight / out must be 16-byte aligned");
  const size_t need = aphro_moe_wna16_gemm_large_workspace_bytes(a_rows, K, a_dtype);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0)) {
    set_error("moe_wna16_gemm_large: workspace %zu < %zu bytes (or not 16-byte aligned)", workspace_bytes, need);
    return APHRO_ERR_WORKSPACE;
  }
  MoeLargeParams p;
  p.a = (const uint16_t*)a; p.lda = (int)lda;
  if (a_dtype == APHRO_BF16) {      // the UN-gathered rows, once per call
    const int64_t n8 = a_rows * K / 8;
    hipLaunchKernelGGL(moe_wna16_large_bf16_to_f16_rows_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st,
                       (const uint16_t*)a, (uint16_t*)workspace, (int)a_rows, (int)K, (int)lda);
    APHRO_LAUNCH_CHECK();
    p.a = (const uint16_t*)workspace; p.lda = (int)K;
  }
  p.sorted = sorted_token_ids; p.expert_ids = expert_ids; p.post_pad = num_tokens_post_pad;
  p.qw = q_weight; p.qz = qzeros; p.sc = (const uint16_t*)scales; p.c = out;
  p.a_rows = (int)a_rows; p.topk = topk;
  p.row_limit = (int)(sorted_token_ids && sorted_len < m_pad ? sorted_len : m_pad);
  p.m_pad = (int)m_pad; p.N = (int)N; p.K = (int)K; p.groups = (int)groups;
  p.gs_tiles = (int)(K / groups / 64);
  p.num_experts = (int)num_experts; p.zero_offset = zero_offset;
  p.out_bf16 = dtype == APHRO_BF16; p.scale_bf16 = dtype == APHRO_BF16; p.mode = mode;
  p.tiles_m = p.tiles_n = 0;
  if (bn == 0) bn = moe_wna16_large_bn(m_pad, N);
  return bn == 256 ? moe_wna16_large_launch<4>(p, st) : moe_wna16_large_launch<2>(p, st);
}
