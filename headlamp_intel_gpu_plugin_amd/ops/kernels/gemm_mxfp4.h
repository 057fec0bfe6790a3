// MXFP4 workload kernels (gfx950 / CDNA4). Part of workload.hip: included
// inside its anonymous namespace after gemm_mxfp8.h, whose vector types and
// dpp helper are used here, as are the tile map, half-tile row assignment
// (p8_src_row), LDS constants and packed epilogue (p8_store_c) of
// gemm_bf16_nt_8ph, all unchanged. The launchers and the two Python bindings
// are at the bottom of this file.
//
//   gemm_mxfp4_nt   C[M,N] = Σ_k (A[m,k]·2^(SA[m,k/32]−127)) · (B[n,k]·2^(SB[n,k/32]−127))
//                   A, B OCP e2m1, two per byte (element 2i in bits 0-3 of
//                   byte i), row-major [rows, K/2] bytes; SA, SB E8M0 bytes
//                   [rows, K/32], mandatory; fp32 accumulate on
//                   v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz:4 blgp:4), bf16
//                   out (RNE). M, N multiples of 256, K of 512 (the schedule
//                   consumes K-tiles in pairs and has no tail).
//   quantize_mxfp4  bf16 [R,K] → packed e2m1 [R,K/2] + E8M0 [R,K/32], OCP MX
//                   rule with emax = 2.
//
// gemm_mxfp4_nt design
//   Tile. 256×256×256, 512 threads, 8 waves as 2×4, 128×64 of C per wave, one
//   block per CU. A K-tile row of 256 e2m1 is 128 bytes, the byte geometry of
//   gemm_bf16_nt_8ph's 64-element row, so tile map, staging and LDS image are
//   that kernel's byte for byte: two K-tiles in LDS, each four 16 KiB
//   half-tiles (A0 A1 B0 B1), every wave writing LDS rows [16·wave, +16) of a
//   half-tile with two global_load_lds_dwordx4, 16-byte chunk c of row r at
//   chunk c ^ (r & 7) by swizzling the per-lane SOURCE address. Per-lane
//   offsets are 32-bit: the host requires M·K/2 and N·K/2 < 2^32.
//   Fragments. With both operands fp4 the MFMA takes 16 bytes per lane per
//   operand (the first four registers of the eight-register operand; the
//   rest are passed undefined): lane l, g = l>>4, holds row l&15 and elements
//   k = 32g .. 32g+31 of the MFMA's 128, one whole MX block. That is logical
//   chunk g of the LDS row for ks = 0 and chunk 4+g for ks = 1: one
//   ds_read_b128 each through the XOR, the ks = 0 / ks = 1 reads of
//   gemm_bf16_nt_8ph (measured conflict-free there). One 128-byte row feeds
//   two MFMAs, as in that kernel, each with four times the flops. The scale
//   operand of lane group g applies to K-block g of the MFMA (the rule
//   gemm_mxfp8.h observed), so here data and scale of a lane belong to the
//   same block: MX block g for ks = 0, 4+g for ks = 1.
//   Scales. A row has 8 scale bytes per K-tile. The 4 KiB of a K-tile (SA of
//   the 256 tile rows, then SB, rows in tile order, 8 bytes each) go through
//   LDS behind the operand buffers (2 slots, 136 KiB in all): thread t stages
//   dword t&1 of tile row t>>1 of SA and of SB with one 4-byte
//   global_load_lds each, so every wave issues the same number of
//   vector-memory operations. A lane fetches the 8 bytes of each row it
//   feeds with one ds_read_b64 next to that row-group's fragment reads (16
//   rows × 8 bytes per lane group, all four groups the same addresses:
//   conflict-free by broadcast), and one v_perm_b32 per row-group, after the
//   wait, leaves byte g in byte 0 and byte 4+g in byte 1 of one register
//   (bytes 2-3 zero); op_sel 0 picks the first for ks = 0 and op_sel 1 the
//   second for ks = 1.
//   Observed on the MI355X: the exact scaled test passes with this fragment
//   map, this scale rule and op_sel reading byte 1, all as expected from the
//   ISA document. In that test SA and SB differ between bytes g and 4+g of a
//   K-tile, between K-tiles and between rows, so either side's wrong byte,
//   slot or row changes the result.
//   Compute. By quadrants, as in gemm_bf16_nt_8ph: a 64×32 quadrant of the
//   wave's 128×64 is 2 (ks) × 4 × 2 MFMAs, operands entered as (B, A) so each
//   lane ends with four consecutive columns of a C row (what p8_store_c
//   packs). Fragments 64 VGPRs, raw scale bytes 16, accumulators 128.
//   Pipeline. The eight-phase order of gemm_bf16_nt_8ph: a phase reads the
//   fragments of one quadrant, issues one half-tile of DMA, then barrier,
//   lgkmcnt(0), 16 MFMAs, barrier; eight phases cover two K-tiles. Wave row 1
//   runs one barrier behind wave row 0 (an extra barrier up front, balanced
//   at the end). Raw s_barrier throughout; vmcnt is never drained in the loop.
//   Staging order (written → phase), with the phases that read it:
//     even buffer, read 1-3:  B0@2 A0@3 B1@4 A1@5, scale slot 0 @5 (K-tile kt+2)
//     odd  buffer, read 5-7:  B0@6 A0@7 B1@8 A1@1, scale slot 1 @1 (kt+1, kt+3)
//   Two rules make a rewrite safe with the wave rows half a phase apart: what
//   is staged in phase p is read by nobody in phase p, and reads of it in
//   phase p−1 are retired before that phase's first barrier. B0 is the one
//   case of the second rule (read in 1, staged in 2): phase 1 issues B's LDS
//   reads, then (behind a sched_barrier) A's, then s_waitcnt lgkmcnt(10),
//   which retires B's because LDS reads return in order. A's reads are 8
//   ds_read_b128, which cannot pair, and 4 ds_read_b64, which the compiler
//   pairs into 2 ds_read2_b64: ten instructions is the FEWEST A can be, and
//   the count must never exceed the number of A's instructions (a larger one
//   would leave B reads outstanding across the barrier: a race). Ten is exact
//   as built; with the b64 unpaired (twelve) the wait is merely two reads
//   early. Do not raise it to 12. The scale slots are read in phases 1-3 / 5-7 and staged in 5 / 1, two phases
//   clear on both sides.
//   Wait counts. Every stage is two DMAs per wave, the scale stage included,
//   and they retire in issue order. The issue order of one trip is
//   A1@1 S@1 B0@2 A0@3 B1@4 | A1@5 S@5 B0@6 A0@7 B1@8. The wait in phase 4
//   follows B1@4: vmcnt(6) leaves B0 A0 B1 of K-tile kt+2 (three half-tiles,
//   6 DMAs) in flight and retires everything older, which is A1@1 and S@1,
//   the last pieces of the odd buffer read from phase 5. The wait in phase 8
//   is the same one half a trip later and completes the even buffer and scale
//   slot 0 for phase 1 of the next trip. Each wait is followed by the two
//   barriers of its phase before the first read, so every wave's wait has
//   been passed. The prologue stages slot 0, K-tile 0 and B0 A0 B1 of K-tile 1
//   and waits vmcnt(6) likewise. Staging past the last K-tile reloads the
//   last one into a buffer that is never read again, so every trip counts the
//   same; a final vmcnt(0) keeps any DMA from outliving the block.

constexpr int P4_SCALES = 2 * 256 * 8;          // scale bytes of one K-tile: SA rows, then SB rows
constexpr int P4_LDS = P8_LDS + 2 * P4_SCALES;  // 136 KiB

__device__ __forceinline__ i32x8 p4_operand(i32x4 v) {  // fp4 uses registers 0-3 only
  return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1);
}

__global__ __launch_bounds__(P8_THREADS) void gemm_mxfp4_nt(const uint8_t* __restrict__ A,
                                                           const uint8_t* __restrict__ B,
                                                           const uint8_t* __restrict__ SA,
                                                           const uint8_t* __restrict__ SB,
                                                           uint16_t* __restrict__ C, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  int m0, n0;
  p8_tile_origin(M, N, m0, n0);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 2;  // 2 wave rows × 4 wave columns
  const int wc = wave & 3;
  const int kb = K / 2;   // bytes per operand row
  const int kq = K / 32;  // scale bytes per row
  const int nk = K / 256;

  // Staging, as in gemm_bf16_nt_8ph: lane l covers LDS row 16·wave + 8s + l/8,
  // physical chunk l%8, loaded from logical chunk (l%8) ^ (row & 7).
  uint32_t src_off[4][2];  // byte offset of this lane's 16 B at k = 0
#pragma unroll
  for (int kind = 0; kind < 4; ++kind)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int r = wave * 16 + s * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ (r & 7);
      const int grow = (kind < 2 ? m0 : n0) + p8_src_row(kind, r);
      src_off[kind][s] = static_cast<uint32_t>(grow) * static_cast<uint32_t>(kb) + chunk * 16;
    }
  // Scales: thread t stages dword t&1 of tile row t>>1; the wave's 64 dwords
  // land lane-linear at byte 256·wave of the slot's SA (and SB) half.
  const uint32_t sc_off = (threadIdx.x >> 1) * static_cast<uint32_t>(kq) + (threadIdx.x & 1) * 4;
  const uint32_t sa_off = static_cast<uint32_t>(m0) * kq + sc_off;
  const uint32_t sb_off = static_cast<uint32_t>(n0) * kq + sc_off;

#define P4_DMA(src, dst, bytes)                                                                            \
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src),                        \
                                   (__attribute__((address_space(3))) void*)(dst), bytes, 0, 0);
#define P4_STAGE(kind, buf, ktile)                                                                         \
  {                                                                                                        \
    const uint32_t kt_ = min((ktile), nk - 1);                                                             \
    const uint8_t* base_ = (kind) < 2 ? A : B;                                                             \
    _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                          \
      P4_DMA(base_ + (src_off[kind][s] + kt_ * 128u),                                                      \
             smem + (buf) * P8_BUF + (kind) * P8_HALF + (wave * 16 + s * 8) * 128, 16)                     \
  }
#define P4_STAGE_SCALES(slot, ktile)                                                                       \
  {                                                                                                        \
    const uint32_t kt_ = min((ktile), nk - 1);                                                             \
    P4_DMA(SA + (sa_off + kt_ * 8u), smem + P8_LDS + (slot) * P4_SCALES + wave * 256, 4)                   \
    P4_DMA(SB + (sb_off + kt_ * 8u), smem + P8_LDS + (slot) * P4_SCALES + 2048 + wave * 256, 4)            \
  }

  // Fragment reads: lane l takes row l&15 of a 16-row group, chunk g + 4·ks
  // through the XOR (row & 7 == frow & 7), and the row's 8 scale bytes.
  const int frow = lane & 15;
  const int g = lane >> 4;
  const int rd0 = (g ^ (frow & 7)) * 16;  // byte offset of ks = 0; ks = 1 is rd0 ^ 64
  const int a_row = wr * 64 + frow;       // LDS row within an A half-tile
  const int b_row = wc * 32 + frow;       // … within a B half-tile
  const int sa_rd = P8_LDS + (wr * 128 + frow) * 8;         // + slot, + 8·(64·mh + 16·mt)
  const int sb_rd = P8_LDS + 2048 + (wc * 64 + frow) * 8;   // + slot, + 8·(32·nh + 16·nt)
  // v_perm_b32 selector: byte g of the low dword, byte g of the high one (= byte 4+g), two zero bytes (0x0c).
  const uint32_t sel = 0x0c0c0400u + g * 0x0101u;

  i32x4 af[8];      // A fragments of one 64-row subtile: [mt*2 + ks]
  i32x4 bq[2][4];   // B fragments of both 32-col subtiles: [nh][nt*2 + ks]
  u32x2 sa_raw[4];  // the 8 scale bytes of each A row-group of that subtile
  u32x2 sb_raw[2][2];
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#define P4_READ_A(buf, mh) /* 8 ds_read_b128 + 4 ds_read_b64 (paired by the compiler) */                                            \
  {                                                                                                        \
    const unsigned char* h_ = smem + (buf) * P8_BUF + (mh) * P8_HALF;                                       \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt) {                                                     \
      const unsigned char* row_ = h_ + (a_row + mt * 16) * 128;                                            \
      af[mt * 2 + 0] = *reinterpret_cast<const i32x4*>(row_ + rd0);                                        \
      af[mt * 2 + 1] = *reinterpret_cast<const i32x4*>(row_ + (rd0 ^ 64));                                 \
      sa_raw[mt] = *reinterpret_cast<const u32x2*>(smem + (buf) * P4_SCALES + sa_rd + ((mh) * 64 + mt * 16) * 8); \
    }                                                                                                      \
  }
#define P4_READ_B(buf, nh) /* 4 ds_read_b128 + 2 ds_read_b64 */                                            \
  {                                                                                                        \
    const unsigned char* h_ = smem + (buf) * P8_BUF + (2 + (nh)) * P8_HALF;                                 \
    _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                                     \
      const unsigned char* row_ = h_ + (b_row + nt * 16) * 128;                                            \
      bq[nh][nt * 2 + 0] = *reinterpret_cast<const i32x4*>(row_ + rd0);                                    \
      bq[nh][nt * 2 + 1] = *reinterpret_cast<const i32x4*>(row_ + (rd0 ^ 64));                             \
      sb_raw[nh][nt] = *reinterpret_cast<const u32x2*>(smem + (buf) * P4_SCALES + sb_rd + ((nh) * 32 + nt * 16) * 8); \
    }                                                                                                      \
  }
// (B, A): the product is the 16×16 tile of Cᵀ, so a lane holds row m = l&15,
// columns 4g..4g+3 of C. The first scale operand belongs to B, the second to A.
#define P4_MFMA_KS(mh, nh, ks)                                                                             \
  _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                         \
  _Pragma("unroll") for (int nt = 0; nt < 2; ++nt)                                                         \
    acc[(mh) * 4 + mt][(nh) * 2 + nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                  \
        p4_operand(bq[nh][nt * 2 + ks]), p4_operand(af[mt * 2 + ks]), acc[(mh) * 4 + mt][(nh) * 2 + nt], 4, 4, ks, \
        sb_[nt], ks, sa_[mt]);
#define P4_MFMA(mh, nh)                                                                                    \
  {                                                                                                        \
    int sa_[4], sb_[2];                                                                                    \
    _Pragma("unroll") for (int mt = 0; mt < 4; ++mt)                                                       \
      sa_[mt] = __builtin_amdgcn_perm(sa_raw[mt][1], sa_raw[mt][0], sel);                                  \
    _Pragma("unroll") for (int nt = 0; nt < 2; ++nt)                                                       \
      sb_[nt] = __builtin_amdgcn_perm(sb_raw[nh][nt][1], sb_raw[nh][nt][0], sel);                          \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    P4_MFMA_KS(mh, nh, 0)                                                                                  \
    P4_MFMA_KS(mh, nh, 1)                                                                                  \
    __builtin_amdgcn_s_setprio(0);                                                                         \
  }
#define P4_SYNC_MFMA(mh, nh)                                                                               \
  __builtin_amdgcn_s_barrier();                                                                            \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                       \
  __builtin_amdgcn_sched_barrier(0);                                                                       \
  P4_MFMA(mh, nh)                                                                                          \
  __builtin_amdgcn_s_barrier();

  // Prologue: scales and K-tile 0 → slot 0 / even buffer, then B0 A0 B1 of
  // K-tile 1 → odd buffer; vmcnt(6) leaves those three in flight.
  P4_STAGE_SCALES(0, 0)
  P4_STAGE(kB0, 0, 0) P4_STAGE(kA0, 0, 0) P4_STAGE(kB1, 0, 0) P4_STAGE(kA1, 0, 0)
  P4_STAGE(kB0, 1, 1) P4_STAGE(kA0, 1, 1) P4_STAGE(kB1, 1, 1)
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();  // stagger the wave rows by one barrier

  for (int it = 0; it < nk / 2; ++it) {
    const int kt = 2 * it;
    // ---- even buffer, scale slot 0: K-tile kt ----
    P4_READ_B(0, 0)
    __builtin_amdgcn_sched_barrier(0);
    P4_READ_A(0, 0)
    P4_STAGE(kA1, 1, kt + 1)
    P4_STAGE_SCALES(1, kt + 1)
    asm volatile("s_waitcnt lgkmcnt(10)" ::: "memory");  // retire the B reads before the barrier
    P4_SYNC_MFMA(0, 0)
    P4_READ_B(0, 1)
    P4_STAGE(kB0, 0, kt + 2)
    P4_SYNC_MFMA(0, 1)
    P4_READ_A(0, 1)
    P4_STAGE(kA0, 0, kt + 2)
    P4_SYNC_MFMA(1, 1)
    P4_STAGE(kB1, 0, kt + 2)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // odd buffer and slot 1 (K-tile kt+1) complete
    P4_SYNC_MFMA(1, 0)
    // ---- odd buffer, scale slot 1: K-tile kt+1 ----
    P4_READ_B(1, 0)
    __builtin_amdgcn_sched_barrier(0);
    P4_READ_A(1, 0)
    P4_STAGE(kA1, 0, kt + 2)
    P4_STAGE_SCALES(0, kt + 2)
    asm volatile("s_waitcnt lgkmcnt(10)" ::: "memory");
    P4_SYNC_MFMA(0, 0)
    P4_READ_B(1, 1)
    P4_STAGE(kB0, 1, kt + 3)
    P4_SYNC_MFMA(0, 1)
    P4_READ_A(1, 1)
    P4_STAGE(kA0, 1, kt + 3)
    P4_SYNC_MFMA(1, 1)
    P4_STAGE(kB1, 1, kt + 3)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // even buffer and slot 0 (K-tile kt+2) complete
    P4_SYNC_MFMA(1, 0)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the block
  if (wr == 0) __builtin_amdgcn_s_barrier();        // balance the stagger barrier
#undef P4_DMA
#undef P4_STAGE
#undef P4_STAGE_SCALES
#undef P4_READ_A
#undef P4_READ_B
#undef P4_MFMA_KS
#undef P4_MFMA
#undef P4_SYNC_MFMA

  p8_store_c(acc, C, N, m0, n0, wr, wc, lane);
}

// quantize_mxfp4: quantize_mxfp8's structure, 16 bytes (8 bf16) per lane, four
// lanes per MX block of 32, one dword of eight e2m1 codes out per lane. Per
// block X = floor(log2(amax)) − 2 clamped to [−127, 127], scale byte X + 127,
// element RNE_e2m1(clamp(v·2^−X, ±6)); an all-zero block gets scale byte 127.
// With e the exponent field of amax: scale byte = max(e − 2, 0), and 2^−X is
// the float with exponent field 254 − scale byte (2..254: normal), an exact
// multiply. The encoding is plain arithmetic, not the fp4 convert
// instruction: x = min(|v|·2^−X, 6) lies in one of three ranges of the e2m1
// grid {0 .5 1 1.5 | 2 3 | 4 6} with steps ½, 1, 2, and adding 2^22, 2^23 or
// 2^24 makes the fp32 add itself round x to a multiple of that step, nearest
// even. The low mantissa bits are then x/step, and the code is that count
// plus 0, 2 or 4; an even count is an even code, so ties go to the even e2m1
// mantissa, and a carry into the next range lands on its first code. The sign
// bit of v is copied: a negative value that rounds to zero becomes −0 (0x8).
__attribute__((target("no-packed-fp32-ops")))
__global__ __launch_bounds__(256) void quantize_mxfp4(const u32x4* __restrict__ x, uint32_t* __restrict__ q,
                                                      uint8_t* __restrict__ scales, size_t n8) {
  // n8 (16-byte vectors) is a multiple of 4: a block's four lanes are in or
  // out of range together; lanes past the end only skip the memory accesses.
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool live = t < n8;
  const u32x4 raw = live ? x[t] : u32x4{0, 0, 0, 0};
  uint32_t bits[8];
  uint32_t amax = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    bits[2 * p] = raw[p] << 16;  // bf16 → fp32 is a shift
    bits[2 * p + 1] = raw[p] & 0xffff0000u;
    amax = max(amax, max(bits[2 * p] & 0x7fffffffu, bits[2 * p + 1] & 0x7fffffffu));
  }
  amax = max(amax, dpp<0xB1>(amax));  // quad_perm:[1,0,3,2]
  amax = max(amax, dpp<0x4E>(amax));  // quad_perm:[2,3,0,1]
  const uint32_t e = amax >> 23;
  const uint32_t sbyte = amax == 0 ? 127u : (e > 2 ? e - 2 : 0u);
  const float inv = __builtin_bit_cast(float, (254u - sbyte) << 23);
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float ax = fminf(__builtin_bit_cast(float, bits[i] & 0x7fffffffu) * inv, 6.f);
    const float magic = ax < 2.f ? 4194304.f : (ax < 4.f ? 8388608.f : 16777216.f);
    const uint32_t bias = ax < 2.f ? 0u : (ax < 4.f ? 2u : 4u);
    const uint32_t code = (__builtin_bit_cast(uint32_t, ax + magic) & 7u) + bias;
    word |= (code | (bits[i] >> 28 & 8u)) << (4 * i);
  }
  if (live) q[t] = word;

  uint32_t sw = sbyte << (8 * ((threadIdx.x >> 2) & 3));
  sw |= dpp<0x124>(sw);  // row_ror:4
  sw |= dpp<0x128>(sw);  // row_ror:8
  if ((threadIdx.x & 15) == 0 && live) {
    if (t + 16 <= n8) {
      *reinterpret_cast<uint32_t*>(scales + (t >> 2)) = sw;
    } else {  // last, partial group of blocks: byte stores
      for (size_t j = 0; t + 4 * j < n8; ++j) scales[(t >> 2) + j] = static_cast<uint8_t>(sw >> (8 * j));
    }
  }
}

bool g_mxfp4_attr = false;

// No unscaled flavour and no smaller-tile fallback.
const char* launch_gemm_mxfp4(const void* a, const void* b, const void* sa, const void* sb, void* c, int m, int n,
                              int k, hipStream_t stream) {
  if (m <= 0 || n <= 0 || k <= 0 || m % 256 || n % 256 || k % 512 ||
      static_cast<uint64_t>(m) * (k / 2) >= (1ull << 32) || static_cast<uint64_t>(n) * (k / 2) >= (1ull << 32))
    return "gemm_mxfp4_nt: needs M,N multiples of 256, K of 512, M*K/2 and N*K/2 < 2^32";
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
    return "gemm_mxfp4_nt: A, B and C must be 16-byte aligned";
  if (sa == nullptr || sb == nullptr) return "gemm_mxfp4_nt: both scale tensors are required";
  if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) & 3)
    return "gemm_mxfp4_nt: scales must be 4-byte aligned";
  if (!g_mxfp4_attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_mxfp4_nt), hipFuncAttributeMaxDynamicSharedMemorySize,
                            P4_LDS) != hipSuccess)
      return "gemm_mxfp4_nt: cannot reserve LDS";
    g_mxfp4_attr = true;
  }
  hipLaunchKernelGGL(gemm_mxfp4_nt, dim3((m / 256) * (n / 256)), dim3(P8_THREADS), P4_LDS, stream,
                     static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<const uint8_t*>(sa),
                     static_cast<const uint8_t*>(sb), static_cast<uint16_t*>(c), m, n, k);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? nullptr : hipGetErrorString(err);
}

const char* launch_quantize_mxfp4(const void* x, void* q, void* scales, long long rows, long long k,
                                  hipStream_t stream) {
  if (rows <= 0 || k <= 0 || k % 32) return "quantize_mxfp4: needs rows > 0 and K a positive multiple of 32";
  if ((reinterpret_cast<uintptr_t>(x) & 15) || ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(scales)) & 3))
    return "quantize_mxfp4: x must be 16-byte, q and scales 4-byte aligned";
  if (rows > (1ll << 40) / k) return "quantize_mxfp4: tensor too large for one pass";
  const size_t n8 = static_cast<size_t>(rows) * static_cast<size_t>(k) / 8;
  hipLaunchKernelGGL(quantize_mxfp4, dim3(static_cast<unsigned>((n8 + 255) / 256)), dim3(256), 0, stream,
                     static_cast<const u32x4*>(x), static_cast<uint32_t*>(q), static_cast<uint8_t*>(scales), n8);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? nullptr : hipGetErrorString(err);
}

PyObject* py_gemm_mxfp4(PyObject*, PyObject* args) {
  unsigned long long a, b, sa, sb, c, stream;
  int m, n, k;
  if (!PyArg_ParseTuple(args, "KKKKKiiiK", &a, &b, &sa, &sb, &c, &m, &n, &k, &stream)) return nullptr;
  const char* err = launch_gemm_mxfp4(reinterpret_cast<void*>(a), reinterpret_cast<void*>(b), reinterpret_cast<void*>(sa),
                                      reinterpret_cast<void*>(sb), reinterpret_cast<void*>(c), m, n, k,
                                      reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

PyObject* py_quantize_mxfp4(PyObject*, PyObject* args) {
  unsigned long long x, q, scales, stream;
  long long rows, k;
  if (!PyArg_ParseTuple(args, "KKKLLK", &x, &q, &scales, &rows, &k, &stream)) return nullptr;
  const char* err = launch_quantize_mxfp4(reinterpret_cast<void*>(x), reinterpret_cast<void*>(q),
                                          reinterpret_cast<void*>(scales), rows, k, reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}
