// Decode attention over a bf16 KV cache (gfx950 / CDNA4). Part of workload.hip:
// included inside its anonymous namespace after gemm_mxfp4_skinny.h, whose
// pattern (one streamed operand, few rows, the long axis split over blocks,
// partials merged in a fixed order) it applies to attention. Launcher, checks
// and the Python binding are at the bottom.
//
//   attn_decode          out[b,h,:] = Σ_s softmax_s(scale·q[b,h,:]·k[b,g,s,:]) · v[b,g,s,:]
//                        over s < seq_lens[b], g = h / G the KV head of query
//                        head h. q, out [B,Hq,128] bf16; k, v [B,Hkv,S_max,128]
//                        bf16; Hq = G·Hkv, 1 ≤ G ≤ 16; fp32 accumulation.
//                        split_kv = 1: bf16 out. split_kv > 1: unnormalised
//                        fp32 accumulator, maximum and sum to the workspace,
//                        [split][B][Hq][128] then [split][B][Hq][2].
//   attn_decode_combine  merges the partials in ascending split order with the
//                        max-rescale, skipping those whose sum is 0, rounds
//                        once to bf16. No atomics anywhere: bit-identical reruns.
//
// Work split. Grid (Hkv, B, split_kv), 256 threads. A block owns one
// (sequence, KV head) and a contiguous slice of that sequence's keys: with
// T = ⌈len/32⌉ tiles of AD_TILE = 32 keys and P = ⌈T/split⌉, block z owns tiles
// zP .. min((z+1)P, T)−1, computed from seq_lens[b] on the device, so every
// sequence of a ragged batch splits its own length (a block past the end has
// no tiles and stores maximum −inf, sum 0, accumulator 0). Wave w walks tiles
// w, w+4, … of the slice with its own running maximum m, running sum l and
// accumulator; there is no block barrier in the loop. The G query heads of the
// group are the 16 columns of one MFMA tile, so every K and V byte fetched
// serves G heads: column i ≥ G reads head G−1 (clamped) and is never stored.
//
// Lanes. i = lane & 15, g = lane >> 4. v_mfma_f32_16x16x32_bf16 takes from
// lane (i, g) A[row i][k 8g..8g+7] and B[k 8g..8g+7][col i] and leaves
// D[row 4g+r][col i] in element r of its accumulator.
//
// Scores, Sᵀ = K·Qᵀ. Operands entered as (K, Q): per 16 keys (sub-tile t of a
// tile) four MFMAs over d = 32ks .. +31. A is K: lane (i, g) loads the 16
// bytes at 64ks + 16g of key row kv0 + 16t + i, global → VGPR, no LDS. B is
// Q: the 16 bytes at 64ks + 16g of head min(i, G−1), loaded once per block.
// Lane (i, g) ends with the scores of head i at keys kv0 + 16t + 4g + r,
// r = 0..3: every value a lane holds belongs to one head, so the maximum, the
// sum and the rescale factor are per lane, shared by the lanes i, i+16, i+32,
// i+48 (two xor-shuffles for the maximum; the sum stays a per-lane partial
// until the end). Key rows at or past len load row len−1 (clamped, in
// bounds) and their scores are set to −inf before the maximum.
// Two tiles of K (2 × 8 dwordx4 per lane) are kept in flight in a register
// ring whose slot is the tile's parity, static because the loop is unrolled
// by two. Past the wave's last tile the ring and the V staging go on loading
// the clamped row, so every iteration issues the same count and the counted
// wait below holds; that data is never used. Offsets are 32-bit per lane:
// the host requires B·Hkv·S_max·256 < 2^32.
//
// Softmax. Scores are multiplied by scale·log2(e) in fp32 after the MFMA
// (scaling bf16 Q would round them), online softmax on v_exp_f32. The
// accumulator and the sum are rescaled only when some lane's maximum moved
// (wave vote). While the maximum is −inf (nothing seen) the exponent is
// taken against 0, so no exp2(−inf − (−inf)) is ever formed. P is rounded to
// bf16 (RNE) and the running sum adds those rounded values.
//
// Output, Oᵀ = Vᵀ·Pᵀ on v_mfma_f32_16x16x32_bf16, one per 16 values of d
// (db = 0..7) and tile. B is Pᵀ: k-slot 8g + 4t + r of the MFMA is key
// kv0 + 16t + 4g + r, which is exactly what the lane holds from the score
// MFMAs: P goes from accumulator to operand with four v_cvt_pk, no LDS and
// no cross-lane move. (The 16×16×16 form would take one sub-tile without
// this interleave but twice the instructions for the same work.) A is Vᵀ:
// lane (i, g) needs V[kv0 + 16t + 4g + r][16db + i] in slot 4t + r. V's rows
// are d-contiguous, so V goes through LDS and is read back transposed:
// ds_read_b64_tr_b16 gives lane i of a 16-lane group element e = the
// element i%4 of the 8 bytes addressed by lane 4e + i/4 of the group; lane
// j of group g addresses row 16t + 4g + j/4, d = 16db + 4(j%4), so lane i
// receives rows 16t + 4g + e at d = 16db + i. Lane (i, g) ends with
// Oᵀ[16db + 4g + r][head i]: four consecutive d of one head, one 8-byte bf16
// or one 16-byte fp32 store.
//
// V staging. Each wave stages its own tile (32 rows × 256 bytes = 8 KiB)
// with eight global_load_lds_dwordx4 into a private double buffer: 8 KiB × 2
// × 4 waves = 64 KiB per block, two blocks per CU. DMA q writes LDS bytes
// [1024q, +1024) of the buffer, rows 4q .. 4q+3; lane l covers row
// r = 4q + l/16, physical 16-byte chunk c = l%16, loaded from logical chunk
// c ^ 2(r & 7): the 32-byte block db of row r sits at block db ^ (r & 7).
// The swizzle is on the source address because the DMA writes LDS
// lane-linearly. Conflict-free: a b64 read is served in two halves of 32
// lanes × 8 bytes = all 64 banks once; a half covers g ∈ {0,1} or {2,3},
// eight rows with eight different r & 7 and therefore eight different
// 32-byte blocks, each read by four lanes 8 bytes apart. Unswizzled, the
// eight rows (256 bytes apart) would share one block: 8-way.
// It is wave-local: in iteration j the wave issues K of tile j+2, then the
// DMAs of tile j+1 into the other buffer (whose reads, of tile j−1, are
// complete: their MFMAs have issued), then waits vmcnt(16): what may remain
// in flight is exactly those 8 loads and 8 DMAs, so tile j's V (and tile
// j+1's K, issued before it) has landed. No barrier. The transposing reads
// are inline assembly with their own lgkmcnt wait: given the builtin, the
// compiler, which cannot tell those reads from the DMA writes in flight, puts
// vmcnt(0) before them. It still puts one before the score MFMAs of every
// even tile, because it takes loads and LDS-DMAs to complete out of order
// with each other; there K of tile j+1 and V of tile j are drained early.
//
// End. vmcnt(0) (the trailing clamped DMAs), barrier, every wave writes
// accumulator, m and l to LDS over the V buffers, barrier; wave w then merges
// d = 32w .. 32w+31 of the four states in wave order: M = max m_v,
// f_v = exp2(m_v − M) (0 where m_v = −inf), L = Σ l_v f_v, O = Σ f_v O_v.
// split_kv = 1 stores O/L (0 where L = 0); otherwise O, M and L go to the
// workspace and attn_decode_combine finishes the same way over the splits.
//
// Measured on the MI355X (profiles/attn_decode_ab.md), TB/s over the K and V
// rows below len, q and out, stream_triad 5.74 in the same process:
// B×Hkv×G×S = 32×8×8×8192 5.93-5.95, 64×8×8×2048 5.74-5.76, 1×8×8×8192 1.42
// (split 16, a 34 MB call of two launches), a ragged 16×8×8×8192 batch
// 3.5-3.7: blocks of short sequences finish early and the longest set the time.

constexpr int AD_THREADS = 256;
constexpr int AD_TILE = 32;                             // keys per wave tile
constexpr int AD_LDS = 4 * 2 * AD_TILE * 256;           // 4 waves × double buffer × 8 KiB
constexpr float AD_NEG_INF = -__builtin_huge_valf();

__global__ __launch_bounds__(AD_THREADS) void attn_decode(const uint16_t* __restrict__ Q,
                                                         const unsigned char* __restrict__ K,
                                                         const unsigned char* __restrict__ V,
                                                         const int* __restrict__ seq_lens, uint16_t* __restrict__ O,
                                                         float* __restrict__ W, int G, int s_max, float scale) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15;
  const int g = lane >> 4;
  const int hk = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
  const int Hkv = gridDim.x, B = gridDim.y, split = gridDim.z;
  const int Hq = Hkv * G;

  const int len = min(max(seq_lens[b], 0), s_max);
  const int last = max(len - 1, 0);  // the row that out-of-range keys load
  const int tiles = (len + AD_TILE - 1) / AD_TILE;
  const int per = (tiles + split - 1) / split;
  const int t0 = z * per + wave;                                  // this wave's first tile
  const int t1 = min((z + 1) * per, tiles);                       // end of the block's slice
  const int n = t1 > t0 ? (t1 - t0 + 3) / 4 : 0;                  // this wave's tiles: t0 + 4j
  const uint32_t base = static_cast<uint32_t>(b * Hkv + hk) * static_cast<uint32_t>(s_max) * 256u;
  const float sc = scale * 1.44269504088896340736f;

  // Q fragments: head min(i, G−1) of the group, 16 bytes at 64ks + 16g.
  bf16x8 qf[4];
  {
    const uint16_t* qrow = Q + (static_cast<size_t>(b) * Hq + hk * G + min(i, G - 1)) * 128 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 32 * ks);
  }

  i32x4 kf[2][8];  // [slot][t*4 + ks]
  auto load_k = [&](i32x4(&dst)[8], int j) {
    const int kv0 = (t0 + 4 * j) * AD_TILE;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const uint32_t off = base + static_cast<uint32_t>(min(kv0 + 16 * t + i, last)) * 256u + 16 * g;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) dst[t * 4 + ks] = *reinterpret_cast<const i32x4*>(K + off + 64 * ks);
    }
  };
  unsigned char* const vbuf = smem + wave * (2 * AD_TILE * 256);
  auto stage_v = [&](int buf, int j) {
    const int kv0 = (t0 + 4 * j) * AD_TILE;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = 4 * q + g;  // lane l: row 4q + l/16, physical chunk l%16
      const uint32_t src = base + static_cast<uint32_t>(min(kv0 + r, last)) * 256u + ((i ^ ((r & 7) << 1)) << 4);
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(V + src),
                                       (__attribute__((address_space(3))) void*)(vbuf + buf * (AD_TILE * 256) + q * 1024),
                                       16, 0, 0);
    }
  };
  // Transposing reads: lane j = i of group g addresses row 16t + 4g + j/4, bytes 32·(db ^ (row & 7)) + 8(j%4).
  const int rd_row = 4 * g + (i >> 2);
  uint32_t rd_addr[8];  // LDS address of this lane's 8 bytes in sub-tile 0 of buffer 0, per db
#pragma unroll
  for (int db = 0; db < 8; ++db)
    rd_addr[db] = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(
                      (__attribute__((address_space(3))) unsigned char*)(vbuf))) +
                  rd_row * 256 + ((db ^ (rd_row & 7)) << 5) + ((i & 3) << 3);

  float m = AD_NEG_INF, l = 0.f;
  f32x4 acc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto step = [&](auto slot_c, int j) {
    constexpr int slot = decltype(slot_c)::value;
    const int kv0 = (t0 + 4 * j) * AD_TILE;
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[slot][t * 4 + ks]), qf[ks], s[t],
                                                       0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    load_k(kf[slot], j + 2);
    stage_v(slot ^ 1, j + 1);
    __builtin_amdgcn_sched_barrier(0);

    float mt = AD_NEG_INF;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = kv0 + 16 * t + 4 * g + r < len ? s[t][r] * sc : AD_NEG_INF;
        mt = fmaxf(mt, s[t][r]);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m, mt);
    const float m_ref = m_new == AD_NEG_INF ? 0.f : m_new;  // nothing seen yet: exp2(−inf − 0) = 0, never −inf − −inf
    if (__any(m_new > m)) {
      const float alpha = m_new > m ? __builtin_amdgcn_exp2f(m - m_ref) : 1.f;
      l *= alpha;
#pragma unroll
      for (int db = 0; db < 8; ++db) acc[db] *= alpha;
    }
    m = m_new;
    uint32_t pk[4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t u = pack_bf16x2(__builtin_amdgcn_exp2f(s[t][2 * h] - m_ref),
                                       __builtin_amdgcn_exp2f(s[t][2 * h + 1] - m_ref));
        pk[t * 2 + h] = u;
        l += __builtin_bit_cast(float, u << 16) + __builtin_bit_cast(float, u & 0xffff0000u);
      }
    const bf16x8 pf = __builtin_bit_cast(bf16x8, (u32x4){pk[0], pk[1], pk[2], pk[3]});

    // V of tile j has landed once only the 8 loads and 8 DMAs issued above remain.
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // The reads are inline assembly so that the compiler, which cannot tell these LDS reads from the DMA writes
    // still in flight, does not put its own vmcnt(0) in front of them; their lgkmcnt is therefore waited here.
    u32x2 vf[8][2];  // [db][t]
#pragma unroll
    for (int hb = 0; hb < 8; hb += 4) {
      asm volatile(
          "ds_read_b64_tr_b16 %0, %8 offset:%12\n\tds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
          "ds_read_b64_tr_b16 %2, %9 offset:%12\n\tds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
          "ds_read_b64_tr_b16 %4, %10 offset:%12\n\tds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
          "ds_read_b64_tr_b16 %6, %11 offset:%12\n\tds_read_b64_tr_b16 %7, %11 offset:%13\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(vf[hb][0]), "=&v"(vf[hb][1]), "=&v"(vf[hb + 1][0]), "=&v"(vf[hb + 1][1]), "=&v"(vf[hb + 2][0]),
            "=&v"(vf[hb + 2][1]), "=&v"(vf[hb + 3][0]), "=&v"(vf[hb + 3][1])
          : "v"(rd_addr[hb]), "v"(rd_addr[hb + 1]), "v"(rd_addr[hb + 2]), "v"(rd_addr[hb + 3]),
            "n"(slot * (AD_TILE * 256)), "n"(slot * (AD_TILE * 256) + 16 * 256)
          : "memory");
#pragma unroll
      for (int db = hb; db < hb + 4; ++db)
        acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(bf16x8, (u32x4){vf[db][0][0], vf[db][0][1], vf[db][1][0], vf[db][1][1]}), pf, acc[db],
            0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  if (n > 0) {
    load_k(kf[0], 0);
    load_k(kf[1], 1);
    stage_v(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    for (int j = 0; j < n; j += 2) {
      step(std::integral_constant<int, 0>{}, j);
      if (j + 1 >= n) break;
      step(std::integral_constant<int, 1>{}, j + 1);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // Merge the four waves' states in wave order, over the V buffers.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(smem + wave * 8192 + db * 1024 + lane * 16) = acc[db];
  *reinterpret_cast<f32x2*>(smem + 32768 + wave * 512 + lane * 8) = f32x2{m, l};
  __syncthreads();
  float f[4], M = AD_NEG_INF, L = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) M = fmaxf(M, reinterpret_cast<const f32x2*>(smem + 32768 + v * 512 + lane * 8)[0][0]);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const f32x2 ml = *reinterpret_cast<const f32x2*>(smem + 32768 + v * 512 + lane * 8);
    f[v] = ml[0] == AD_NEG_INF ? 0.f : __builtin_amdgcn_exp2f(ml[0] - M);
    L += ml[1] * f[v];
  }
  const size_t row = static_cast<size_t>(b) * Hq + hk * G + i;  // stored only where i < G
  const size_t rows = static_cast<size_t>(B) * Hq;
  const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int db = 2 * wave + u;
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < 4; ++v) o += f[v] * *reinterpret_cast<const f32x4*>(smem + v * 8192 + db * 1024 + lane * 16);
    if (i >= G) continue;
    const int d = 16 * db + 4 * g;
    if (W == nullptr) {
      o *= inv;
      *reinterpret_cast<u32x2*>(O + row * 128 + d) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
    } else {
      *reinterpret_cast<f32x4*>(W + (z * rows + row) * 128 + d) = o;
    }
  }
  if (W != nullptr && wave == 0 && g == 0 && i < G)
    *reinterpret_cast<f32x2*>(W + static_cast<size_t>(split) * rows * 128 + (z * rows + row) * 2) = f32x2{M, L};
}

// One thread per four consecutive d of one (sequence, head): the split partials
// in ascending order, each rescaled to the running maximum; rows = B·Hq.
__global__ __launch_bounds__(256) void attn_decode_combine(const float* __restrict__ W, uint16_t* __restrict__ O,
                                                           int split, size_t rows) {
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const size_t row = t >> 5;
  if (row >= rows) return;
  const int d = static_cast<int>(t & 31) * 4;
  const float* ML = W + static_cast<size_t>(split) * rows * 128;
  float M = AD_NEG_INF, L = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < split; ++s) {
    const f32x2 ml = *reinterpret_cast<const f32x2*>(ML + (s * rows + row) * 2);
    if (ml[1] == 0.f) continue;  // an empty or fully masked slice
    const float m_new = fmaxf(M, ml[0]);
    const float a = __builtin_amdgcn_exp2f(M - m_new);  // 0 at the first partial taken (M = −inf, m_new finite)
    const float p = __builtin_amdgcn_exp2f(ml[0] - m_new);
    o = o * a + *reinterpret_cast<const f32x4*>(W + (s * rows + row) * 128 + d) * p;
    L = L * a + ml[1] * p;
    M = m_new;
  }
  o *= L > 0.f ? 1.f / L : 0.f;
  *reinterpret_cast<u32x2*>(O + row * 128 + d) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
}

bool g_attn_attr = false;

const char* launch_attn_decode(const void* q, const void* k, const void* v, const void* lens, void* out, int b, int hkv,
                               int g, int s_max, float scale, int split, void* ws, unsigned long long ws_bytes,
                               hipStream_t stream) {
  if (b < 1 || b > 65535 || hkv < 1 || s_max < 1 || split < 1 || split > 65535)
    return "attn_decode_bf16: needs 1 <= B <= 65535, Hkv >= 1, S_max >= 1, 1 <= split_kv <= 65535";
  if (g < 1 || g > 16) return "attn_decode_bf16: needs 1 <= Hq/Hkv <= 16";
  if (static_cast<uint64_t>(b) * hkv * s_max * 256 >= (1ull << 32))
    return "attn_decode_bf16: a cache must be smaller than 2^32 bytes (B*Hkv*S_max*256)";
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return "attn_decode_bf16: q, k_cache, v_cache and out must be 16-byte aligned";
  if (lens == nullptr || (reinterpret_cast<uintptr_t>(lens) & 3)) return "attn_decode_bf16: seq_lens must be 4-byte aligned";
  const size_t rows = static_cast<size_t>(b) * hkv * g;
  if (split > 1) {
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15))
      return "attn_decode_bf16: split_kv > 1 needs a 16-byte aligned workspace";
    if (ws_bytes < static_cast<unsigned long long>(split) * rows * 130 * 4)
      return "attn_decode_bf16: workspace smaller than split_kv*B*Hq*130*4 bytes";
  }
  if (!g_attn_attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(attn_decode), hipFuncAttributeMaxDynamicSharedMemorySize,
                            AD_LDS) != hipSuccess)
      return "attn_decode_bf16: cannot reserve LDS";
    g_attn_attr = true;
  }
  float* w = split > 1 ? static_cast<float*>(ws) : nullptr;
  uint16_t* o16 = static_cast<uint16_t*>(out);
  hipLaunchKernelGGL(attn_decode, dim3(hkv, b, split), dim3(AD_THREADS), AD_LDS, stream,
                     static_cast<const uint16_t*>(q), static_cast<const unsigned char*>(k),
                     static_cast<const unsigned char*>(v), static_cast<const int*>(lens), o16, w, g, s_max, scale);
  if (split > 1)
    hipLaunchKernelGGL(attn_decode_combine, dim3(static_cast<unsigned>((rows * 32 + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const float*>(w), o16, split, rows);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

PyObject* py_attn_decode(PyObject*, PyObject* args) {
  unsigned long long q, k, v, lens, out, ws, ws_bytes, stream;
  int b, hkv, g, s_max, split;
  double scale;
  if (!PyArg_ParseTuple(args, "KKKKKiiiidiKKK", &q, &k, &v, &lens, &out, &b, &hkv, &g, &s_max, &scale, &split, &ws,
                        &ws_bytes, &stream))
    return nullptr;
  const char* err = launch_attn_decode(reinterpret_cast<void*>(q), reinterpret_cast<void*>(k),
                                       reinterpret_cast<void*>(v), reinterpret_cast<void*>(lens),
                                       reinterpret_cast<void*>(out), b, hkv, g, s_max, static_cast<float>(scale), split,
                                       reinterpret_cast<void*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

constexpr const char* kAttnDecodeDoc =
    "attn_decode_bf16(q, k_cache, v_cache, seq_lens, out, B, Hkv, G, S_max, scale, split_kv, workspace, "
    "workspace_bytes, stream): softmax(scale q k^T) v per sequence and query head over a bf16 KV cache "
    "[B,Hkv,S_max,128], Hq = G*Hkv, keys split over split_kv blocks; fp32 partials in workspace "
    "(split_kv*B*Hq*130*4 bytes) merged in order when split_kv > 1.";
