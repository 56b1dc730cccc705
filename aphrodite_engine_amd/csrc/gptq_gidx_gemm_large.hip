// W4A16 GEMM on CHECKPOINT-ORDER GPTQ weights with a per-row group map (g_idx) for PROMPT-sized M on gfx950:
//   c[M, N] = a[M, K] . W,  W[k][n] = (q[k][n] - (qzero[g_idx[k]][n] + zero_offset)) * scale[g_idx[k]][n]
// q_weight int32 [K/8, N] (word r of column n = k 8r .. 8r+7, nibble i = k 8r + i), qzeros int32 [G, N/8], scales [G, N]
// f16 | bf16, g_idx int32 [K]; G is the group count of the UNSHARDED matrix (no relation to K).  Serves the rows above the
// decode kernel (gptq_gidx_gemm.hip, <= 64 rows) where the form used to be reconstructed to [K, N] + a library GEMM.
//
// Design (DESIGN.md "gptq_gidx_gemm_large"):
//   * Operands: D^T[n][m] = W^T[n][k] . A^T[k][m] with v_mfma_f32_32x32x16_f16.  A lane's weight operand (row n = lane & 31,
//     k = 8 (lane >> 5) .. +7 of the 16-k step) is exactly ONE checkpoint word: the packed weights need no transposing
//     layout (the arrangement of gptq8_gemm_large.hip with one word per lane).  The activations are the B operand (lane:
//     column m = lane & 31) and arrive from HBM untouched, so the fragment keeps the NATURAL k order (the decode kernel's
//     0,4,1,5.. order would need the activations re-ordered inside their 16-byte pieces, which a direct-to-LDS load cannot).
//   * A wave's two 32-column MFMA blocks are INTERLEAVED: block nb, MFMA row i = column 2 i + nb of the wave's 64.  A lane
//     then owns two ADJACENT columns: its two packed words are one ds_read_b64, the two scales of a row one ds_read_b32,
//     the two zeros one ds_read_u16 -- and its accumulators are 8 consecutive output columns.
//   * Per-row dequantisation in REGISTERS, per wave, one fragment reused over 4 m-blocks (wave tile 128 rows x 64 columns).
//     Per k-step (16 k) and lane: 8 group ids (two broadcast ds_read_b128), 8 + 8 table reads, one b64 of weights, four
//     b128 of activations; per 8 weights 4 VALU for the nibbles (2 shared and/shift + 4 v_perm + 4 v_or = 11 per word), 4
//     v_perm for the scales, 4 v_perm + 4 v_or for the zeros, 4 packed subtracts, 4 packed multiplies = 31 VALU, plus 12
//     per row pair of columns for clamping g_idx and forming the two table addresses.  (1024 + q) - (1024 + z) is exact in
//     f16 and the multiply by the scale is the only rounding: with f16 scales the MFMA operand has the bits of
//     aphro_gptq_dequant.
//   * The scale / zero table of the workgroup's 128 columns holds ALL G groups in LDS as COMPACT entries -- f16 scale
//     [G][128] + 8-bit zero (zero point + zero_offset, 0..16) [G][128] = 384 bytes per group, 84 KiB at G = 224 -- built once
//     per workgroup.  GXL_MAX_GROUPS = 232 is what fits beside the pipeline; beyond it _supported returns 0.  g_idx is
//     clamped to [0, G - 1]: a bad entry gives wrong numbers, never an out-of-range read.
//   * Data movement: activations, packed weights AND the K tile's 32 g_idx values go global -> LDS with direct-to-LDS
//     loads.  Activations: 64-byte rows XOR-swizzled on the SOURCE address (slot ^ ((row >> 1) & 3)).  4 stages of
//     K tile 32: loads run three tiles ahead, one raw barrier per tile.
//   * Work split: workgroup = 2 x 2 waves, tile 256 rows x 128 columns.  XCD-aware tile order.  Small grids: K is cut into
//     up to 16 slices of whole K tiles (blockIdx.y); every slice writes an fp32 slab and gxl_splitk_reduce_kernel adds the
//     slabs in slice order -- deterministic, no flags, no tickets, no atomics, nothing to reset between HIP-graph replays.
//   * bf16 callers: activations widened to f16 with saturation into the workspace, scales converted to f16 when the table
//     is built, fp32 accumulators, output rounded once to bf16.
#include "common.h"

namespace aphro {

typedef float gxl_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* gxl_lds_ptr;

constexpr int GXL_BM = 256, GXL_BN = 128, GXL_BK = 32, GXL_NST = 4, GXL_NWAVE = 4;
constexpr int GXL_A_STAGE = GXL_BM * GXL_BK * 2;               // bytes: 256 rows x 64 B
constexpr int GXL_B_STAGE = (GXL_BK / 8) * GXL_BN * 4;         // 4 packed rows
constexpr int GXL_G_STAGE = 256;                               // one direct-to-LDS instruction is 64 lanes x 4 bytes: the tile's 32
                                                               // g_idx values + the next 32 (unused; past K the descriptor gives 0)
constexpr int GXL_STAGE = GXL_A_STAGE + GXL_B_STAGE + GXL_G_STAGE;
constexpr int GXL_TAB_ROW = GXL_BN * 3;                        // bytes per group: 128 f16 scales + 128 zero bytes
constexpr int GXL_LDS_MAX = 160 * 1024;
constexpr int GXL_MAX_GROUPS = (GXL_LDS_MAX - GXL_NST * GXL_STAGE) / GXL_TAB_ROW;   // 232
constexpr int gxl_lds_bytes(int groups) { return groups * GXL_TAB_ROW + GXL_NST * GXL_STAGE; }
static_assert(GXL_NST * GXL_STAGE >= GXL_NWAVE * 16384, "the epilogue's transpose regions overlay the LDS");
static_assert(GXL_MAX_GROUPS >= 224, "a 70B down_proj at group 128 has 224 groups");

struct GidxLargeParams {
  const uint16_t* a;       // [M, lda] f16
  const uint32_t* qw;      // [K/8, N] checkpoint order
  const uint32_t* qz;      // [G, N/8]
  const uint16_t* sc;      // [G, N] f16 (or bf16: scale_bf16)
  const int32_t* g_idx;    // [K]
  uint16_t* c;             // [M, N]
  float* partial;          // [ksplit][M][N]
  int M, N, K, G, lda, zero_offset;
  int out_bf16, scale_bf16;
  int tiles_m, tiles_n;
  int ksplit;              // > 1: blockIdx.y owns K / ksplit consecutive k and writes slab blockIdx.y of `partial`
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t gxl_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// One checkpoint word (8 consecutive k of one column) -> 8 scaled f16 in k order: ((1024 + q) - (1024 + z)) * s.
// sr[kk]: the scales of row kk for the lane's column pair (low / high half); zr[kk]: their zeros (byte 0 / byte 1).
template <int NB>
__device__ __forceinline__ f16x8 gxl_dequant(uint32_t w, const uint32_t (&sr)[8], const uint32_t (&zr)[8]) {
  const uint32_t ev = w & 0x0f0f0f0fu, od = (w >> 4) & 0x0f0f0f0fu;       // bytes: q0 q2 q4 q6 / q1 q3 q5 q7
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first, 0x0c = 0x00
    const uint32_t q = __builtin_amdgcn_perm(od, ev, 0x0c000c00u | (uint32_t)j | ((uint32_t)(4 + j) << 16)) | 0x64006400u;
    const uint32_t z = __builtin_amdgcn_perm(zr[2 * j + 1], zr[2 * j], NB ? 0x0c050c01u : 0x0c040c00u) | 0x64006400u;
    const uint32_t s = __builtin_amdgcn_perm(sr[2 * j + 1], sr[2 * j], NB ? 0x07060302u : 0x05040100u);
    const f16x2 d = (__builtin_bit_cast(f16x2, q) - __builtin_bit_cast(f16x2, z)) * __builtin_bit_cast(f16x2, s);
    r[j] = __builtin_bit_cast(uint32_t, d);
  }
  return __builtin_bit_cast(f16x8, r);
}

__global__ __launch_bounds__(GXL_NWAVE * 64) void gptq_gidx_gemm_large_kernel(GidxLargeParams p) {
  constexpr int NT = GXL_NWAVE * 64, BM = GXL_BM, BN = GXL_BN, BK = GXL_BK;
  extern __shared__ __attribute__((aligned(16))) unsigned char gxl_smem[];
  // [scales: G x 128 f16] [zeros: G x 128 bytes] [4 x (A tile | B tile | g_idx)]
  uint16_t* tab_s = reinterpret_cast<uint16_t*>(gxl_smem);
  unsigned char* tab_z = gxl_smem + (size_t)p.G * (BN * 2);
  unsigned char* stages = gxl_smem + (size_t)p.G * GXL_TAB_ROW;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
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
  const __amdgpu_buffer_rsrc_t ra = gxl_rsrc(p.a, (uint32_t)((size_t)p.M * p.lda * 2));
  const __amdgpu_buffer_rsrc_t rb = gxl_rsrc(p.qw, (uint32_t)((size_t)(p.K >> 3) * p.N * 4));
  const __amdgpu_buffer_rsrc_t rg = gxl_rsrc(p.g_idx, (uint32_t)((size_t)p.K * 4));   // (reads past K return 0; never used)

  // ---- staging (direct-to-LDS) ---------------------------------------------------------------------------------------
  // A tile: BM rows x 64 B; one DMA instruction = 16 rows (lane -> row l/4, 16-byte slot l%4).  LDS slot s' of row r holds
  // global slot s' ^ f(r), f(r) = (r >> 1) & 3.  Rows past M re-read row M - 1 (their results are never stored).
  constexpr int A_PER_WAVE = BM / 16 / GXL_NWAVE;              // 4
  int a_voff[A_PER_WAVE];
#pragma unroll
  for (int i = 0; i < A_PER_WAVE; ++i) {
    const int row = (wave * A_PER_WAVE + i) * 16 + (lane >> 2);
    const int slot = (lane & 3) ^ ((row >> 1) & 3);
    a_voff[i] = (int)(((uint32_t)min(m0 + row, p.M - 1) * (uint32_t)p.lda + (uint32_t)slot * 8u) * 2u);
  }
  // B tile: 4 packed rows x BN words; one DMA instruction = 64 words (4 bytes per lane), lane-linear
  constexpr int B_PER_WAVE = GXL_B_STAGE / 256 / GXL_NWAVE;    // 2
  const int b_row_bytes = p.N * 4;
  int b_voff[B_PER_WAVE];
#pragma unroll
  for (int i = 0; i < B_PER_WAVE; ++i) {
    const int bi = wave * B_PER_WAVE + i;
    b_voff[i] = (n0 + (bi & 1) * 64 + lane) * 4 + (bi >> 1) * b_row_bytes;
  }
  const int g_voff = lane * 4;
  auto stage = [&](int st, int kt) {
    unsigned char* sa = stages + st * GXL_STAGE;
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
      const int voff = a_voff[i];       // (a local copy: see wna16_gemm_large.hip on hipcc dropping the host stub otherwise)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (gxl_lds_ptr)(sa + (wave * A_PER_WAVE + i) * 1024), 16, voff,
                                               (k_begin + kt * BK) * 2, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
      const int voff = b_voff[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (gxl_lds_ptr)(sa + GXL_A_STAGE + (wave * B_PER_WAVE + i) * 256), 4, voff,
                                               (k_begin / 8 + kt * (BK / 8)) * b_row_bytes, 0, 0);
    }
    // the tile's g_idx values: every wave writes the same 256 bytes (same values) -- all waves issue the same number of loads
    {
      const int voff = g_voff;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (gxl_lds_ptr)(sa + GXL_A_STAGE + GXL_B_STAGE), 4, voff,
                                               (k_begin + kt * BK) * 4, 0, 0);
    }
  };
  constexpr int DMA_PER_TILE = A_PER_WAVE + B_PER_WAVE + 1;    // per wave and K tile: the counted waits below rely on it
  stage(0, 0);
  if (ktiles > 1) stage(1, 1);
  if (ktiles > 2) stage(2, 2);

  // ---- the tile's scale / zero columns of every group.  unit = (group, 8 columns): one zero-point word + 16 bytes of scales
  const int units = p.G * (BN / 8);
  for (int u = tid; u < units; u += NT) {
    const int grp = u >> 4, cb = u & 15;
    const uint32_t zw = p.qz[(size_t)grp * (p.N >> 3) + (n0 >> 3) + cb];
    u16x8 s8 = *reinterpret_cast<const u16x8*>(p.sc + (size_t)grp * p.N + n0 + 8 * cb);
    if (p.scale_bf16) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s8[e] = bf16_bits_to_f16_bits_sat(s8[e]);
    }
    uint32_t z0 = 0, z1 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      z0 |= (((zw >> (4 * i)) & 0xfu) + (uint32_t)p.zero_offset) << (8 * i);
      z1 |= (((zw >> (4 * i + 16)) & 0xfu) + (uint32_t)p.zero_offset) << (8 * i);
    }
    *reinterpret_cast<u16x8*>(tab_s + (size_t)u * 8) = s8;
    *reinterpret_cast<u32x2*>(tab_z + (size_t)u * 8) = u32x2{z0, z1};
  }
  __syncthreads();

  gxl_f32x16 acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

  // (a wave whose 128 rows are all past M computes on re-read rows and stores nothing: skipping it inside the loop made hipcc
  // move the 128 accumulators between AGPRs and VGPRs every K tile)
  const int zl = wn * 64 + 2 * l31;                            // the lane's column pair inside the workgroup tile
  const int gmax = p.G - 1;
  for (int kt = 0; kt < ktiles; ++kt) {
    const int st = kt % GXL_NST;
    // tile kt has landed once at most the loads of tiles kt + 1, kt + 2 are outstanding; a raw barrier publishes it to every
    // wave and tells everyone that stage (kt + 3) % 4 -- read during tile kt - 1 -- is free
    if (kt + 2 < ktiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * DMA_PER_TILE) : "memory");
    else if (kt + 1 < ktiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(DMA_PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 3 < ktiles) stage((kt + 3) % GXL_NST, kt + 3);
    const unsigned char* sa = stages + st * GXL_STAGE;
    const uint32_t* sb = reinterpret_cast<const uint32_t*>(sa + GXL_A_STAGE);
    const int32_t* sg = reinterpret_cast<const int32_t*>(sa + GXL_A_STAGE + GXL_B_STAGE);
#pragma unroll
    for (int j = 0; j < BK / 16; ++j) {
      const u32x4 g0 = *reinterpret_cast<const u32x4*>(sg + 16 * j + 8 * kh);
      const u32x4 g1 = *reinterpret_cast<const u32x4*>(sg + 16 * j + 8 * kh + 4);
      const int gi[8] = {(int)g0[0], (int)g0[1], (int)g0[2], (int)g0[3], (int)g1[0], (int)g1[1], (int)g1[2], (int)g1[3]};
      uint32_t sr[8], zr[8];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int za = min(max(gi[kk], 0), gmax) * BN + zl;    // zero byte pair; the scale pair sits at twice the offset
        zr[kk] = *reinterpret_cast<const uint16_t*>(tab_z + za);
        sr[kk] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const unsigned char*>(tab_s) + 2 * za);
      }
      const u32x2 w = *reinterpret_cast<const u32x2*>(sb + (2 * j + kh) * BN + zl);
      u32x4 af[4];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int row = wm * 128 + mb * 32 + l31;
        const int slot = (2 * j + kh) ^ ((row >> 1) & 3);
        af[mb] = *reinterpret_cast<const u32x4*>(sa + row * 64 + slot * 16);
      }
      const f16x8 wf0 = gxl_dequant<0>(w[0], sr, zr), wf1 = gxl_dequant<1>(w[1], sr, zr);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        acc[0][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf0, __builtin_bit_cast(f16x8, af[mb]), acc[0][mb], 0, 0, 0);
        acc[1][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf1, __builtin_bit_cast(f16x8, af[mb]), acc[1][mb], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                  // every wave is done with the table and the stage buffers

  // ---- lane holds, for row m = mb * 32 + l31, the 8 consecutive columns 16 q + 8 kh + 2 r + nb (r = 0..3) ----------------
  if (p.ksplit > 1) {                               // fp32 slab of this K range; summed by gxl_splitk_reduce_kernel
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int row = m0 + wm * 128 + mb * 32 + l31;
      if (row >= p.M) continue;
      float* prow = p.partial + ((size_t)blockIdx.y * p.M + row) * p.N + n0 + wn * 64 + 8 * kh;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<f32x4*>(prow + 16 * q) =
            f32x4{acc[0][mb][4 * q], acc[1][mb][4 * q], acc[0][mb][4 * q + 1], acc[1][mb][4 * q + 1]};
        *reinterpret_cast<f32x4*>(prow + 16 * q + 4) =
            f32x4{acc[0][mb][4 * q + 2], acc[1][mb][4 * q + 2], acc[0][mb][4 * q + 3], acc[1][mb][4 * q + 3]};
      }
    }
    return;
  }
  unsigned char* region = gxl_smem + wave * 16384;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float v0 = acc[0][mb][4 * q + 2 * h], v1 = acc[1][mb][4 * q + 2 * h];
        const float v2 = acc[0][mb][4 * q + 2 * h + 1], v3 = acc[1][mb][4 * q + 2 * h + 1];
        epi_put(region, mb * 32 + l31, 4 * q + 2 * kh + h,
                p.out_bf16 ? u32x2{pack2_16<true>(v0, v1), pack2_16<true>(v2, v3)} : u32x2{pack2_16<false>(v0, v1), pack2_16<false>(v2, v3)});
      }
  const int64_t origin = (int64_t)(m0 + wm * 128) * p.N + n0 + wn * 64;      // (elements); rows past M: dropped by the descriptor
  epi_flush_buf(region, p.c + origin, p.N, ((int64_t)p.M * p.N - origin) * 2, lane);
}

// partial [S][M*N] fp32 -> c [M*N] f16 / bf16 (fixed summation order: deterministic)
__global__ void gxl_splitk_reduce_kernel(const float* __restrict__ partial, uint16_t* __restrict__ c, int64_t mn, int S,
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
__global__ void gxl_bf16_to_f16_rows_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int M, int K, int lda) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= (int64_t)M * K) return;
  const int row = (int)(i / K), col = (int)(i % K);
  u16x8 v = *reinterpret_cast<const u16x8*>(in + (size_t)row * lda + col);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f16_bits_sat(v[j]);
  *reinterpret_cast<u16x8*>(out + i) = v;
}

}  // namespace aphro

using namespace aphro;

// One workgroup per (256 x 128 tile, K slice); the table fills the LDS, so one workgroup per CU.  K is cut, on K-tile
// boundaries and no finer than 256, until about one workgroup per CU exists -- as long as the fp32 slabs stay small beside
// the weights.  Every slice builds the table of its columns again (at most 84 KiB from L2).
static int gxl_ksplit(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + GXL_BM - 1) / GXL_BM) * (N / GXL_BN);
  const int64_t slab = M * N * 4;
  int ks = 1;
  for (int s = 2; s <= 16; ++s) {
    if (tiles * ks >= 256) break;
    if (K % (s * GXL_BK) == 0 && K / s >= 256 && s * slab <= (36ll << 20)) ks = s;
  }
  return ks;
}

extern "C" int aphro_gptq_gemm_gidx_large_supported(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (dtype != APHRO_F16 && dtype != APHRO_BF16) return 0;
  if (M < 1 || N < GXL_BN || N % GXL_BN != 0 || K < GXL_BK || K % GXL_BK != 0 || groups < 1 || groups > GXL_MAX_GROUPS) return 0;
  const uint64_t lim = 0xffffffffull;      // every byte offset the kernel forms is 32-bit
  if ((uint64_t)M * K * 2 >= lim || (uint64_t)K * N / 2 >= lim || (uint64_t)M * N * 2 >= lim || (uint64_t)K * 4 >= lim) return 0;
  return 1;
}

extern "C" size_t aphro_gptq_gemm_gidx_large_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (!aphro_gptq_gemm_gidx_large_supported(M, N, K, groups, dtype)) return 0;
  const int ks = gxl_ksplit(M, N, K);
  const size_t b = dtype == APHRO_BF16 ? ((size_t)M * K * 2 + 255) / 256 * 256 : 0;
  return b + (ks > 1 ? (size_t)ks * M * N * sizeof(float) : 0);
}

extern "C" int aphro_gptq_gemm_gidx_large(const void* a, int64_t lda, const uint32_t* q_weight, const uint32_t* qzeros,
                                          const void* scales, const int32_t* g_idx, void* c, void* workspace,
                                          size_t workspace_bytes, int64_t M, int64_t N, int64_t K, int64_t groups,
                                          int zero_offset, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return APHRO_OK;
  APHRO_CHECK(aphro_gptq_gemm_gidx_large_supported(M, N, K, groups, dtype),
              "gptq_gemm_gidx_large: M=%ld N=%ld K=%ld groups=%ld dtype=%d is not served (N %% 128, K %% 32, groups <= %d, operands < 4 GiB)",
              (long)M, (long)N, (long)K, (long)groups, dtype, GXL_MAX_GROUPS);
  APHRO_CHECK(a && q_weight && qzeros && scales && g_idx && c, "gptq_gemm_gidx_large: null tensor");
  APHRO_CHECK(lda >= K && lda % 8 == 0 && ((uintptr_t)a % 16) == 0, "gptq_gemm_gidx_large: a must be 16-byte aligned with lda %% 8 == 0, lda >= K");
  APHRO_CHECK((uint64_t)M * lda * 2 < 0xffffffffull, "gptq_gemm_gidx_large: activations exceed 4 GiB");
  APHRO_CHECK(((uintptr_t)q_weight % 16) == 0 && ((uintptr_t)qzeros % 4) == 0 && ((uintptr_t)scales % 16) == 0 &&
              ((uintptr_t)g_idx % 4) == 0 && ((uintptr_t)c % 16) == 0,
              "gptq_gemm_gidx_large: q_weight, scales and c must be 16-byte aligned");
  APHRO_CHECK(zero_offset == 0 || zero_offset == 1, "gptq_gemm_gidx_large: zero_offset must be 0 or 1");
  const int ks = gxl_ksplit(M, N, K);
  const size_t need = aphro_gptq_gemm_gidx_large_workspace_bytes(M, N, K, groups, dtype);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0)) {
    set_error("gptq_gemm_gidx_large: workspace %zu < %zu bytes (or not 16-byte aligned)", workspace_bytes, need);
    return APHRO_ERR_WORKSPACE;
  }
  GidxLargeParams p;
  p.a = (const uint16_t*)a; p.lda = (int)lda;
  char* ws = (char*)workspace;
  if (dtype == APHRO_BF16) {
    const int64_t n8 = M * K / 8;
    hipLaunchKernelGGL(gxl_bf16_to_f16_rows_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const uint16_t*)a,
                       (uint16_t*)ws, (int)M, (int)K, (int)lda);
    APHRO_LAUNCH_CHECK();
    p.a = (const uint16_t*)ws; p.lda = (int)K;
    ws += ((size_t)M * K * 2 + 255) / 256 * 256;
  }
  p.qw = q_weight; p.qz = qzeros; p.sc = (const uint16_t*)scales; p.g_idx = g_idx; p.c = (uint16_t*)c;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.G = (int)groups; p.zero_offset = zero_offset;
  p.out_bf16 = dtype == APHRO_BF16; p.scale_bf16 = dtype == APHRO_BF16;
  p.tiles_m = (int)((M + GXL_BM - 1) / GXL_BM); p.tiles_n = (int)(N / GXL_BN);
  p.ksplit = ks; p.partial = (float*)ws;
  static bool attr_set_dev[APHRO_MAX_DEVICES] = {}; bool& attr_set = attr_set_dev[device_slot()];
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)gptq_gidx_gemm_large_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GXL_LDS_MAX) != hipSuccess) {
      set_error("gptq_gemm_gidx_large: cannot raise the dynamic LDS limit");
      return APHRO_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(gptq_gidx_gemm_large_kernel, dim3(p.tiles_m * p.tiles_n, p.ksplit), dim3(GXL_NWAVE * 64),
                     (size_t)gxl_lds_bytes(p.G), st, p);
  APHRO_LAUNCH_CHECK();
  if (ks > 1) {
    const int64_t mn = M * N;
    hipLaunchKernelGGL(gxl_splitk_reduce_kernel, dim3((unsigned)((mn / 4 + 255) / 256)), dim3(256), 0, st, p.partial,
                       (uint16_t*)c, mn, ks, p.out_bf16);
    APHRO_LAUNCH_CHECK();
  }
  return APHRO_OK;
}
