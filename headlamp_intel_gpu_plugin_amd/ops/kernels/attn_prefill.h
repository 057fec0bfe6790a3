// Prefill attention over a bf16 KV cache (gfx950 / CDNA4). Part of workload.hip:
// included inside its anonymous namespace after attn_decode.h, whose cache
// layout, transposed products, softmax and V swizzle it keeps, and whose data
// movement it replaces: a key tile here serves 128 query rows, so K and V go
// through LDS once per block and are shared by its four waves. Launcher,
// checks and the Python binding are at the bottom.
//
//   attn_prefill  out[b,i,h,:] = Σ_s softmax_s(scale·q[b,i,h,:]·k[b,h/G,s,:]) · v[b,h/G,s,:]
//                 over the keys s ≤ p, p = seq_lens[b] − Sq + i the position of
//                 query row i (bottom-right aligned causal mask). q, out
//                 [B,Sq,Hq,128] bf16; k, v [B,Hkv,S_max,128] bf16; Hq = G·Hkv,
//                 any G ≥ 1; fp32 accumulation. A row with p < 0 (left padding
//                 of a prompt shorter than Sq) sees no key and stores 0. No
//                 atomics, no split, no workspace: bit-identical reruns.
//
// Work split. One-dimensional grid of B·Hq·⌈Sq/128⌉ blocks of 256 threads. A
// block owns one (sequence, query head) and AP_ROWS = 128 query rows; wave w
// owns rows 32w .. 32w+31 as two MFMA column tiles (rt = 0, 1). The block id
// decomposes, fastest first, into the head within its KV group, the KV head,
// the sequence and the query tile counted from the last: the G blocks that
// stream the same K and V are neighbours in launch order and meet in L2, and
// the tiles with the most visible keys (causal work per tile is triangular)
// start first, so the short ones fill the tail. With p_last the position of
// the block's last row below Sq, the block walks the key tiles of
// AP_TILE = 64 keys 0 .. ⌊p_last/64⌋ and never touches a tile wholly in the
// future (none at all when p_last < 0). A wave whose own last row ends in an
// earlier tile skips the MFMAs of the later ones but still stages its share
// of them and takes the barrier. Only tiles that the diagonal crosses for
// this wave (64j + 63 > position of the wave's first row) are masked, per
// element, against min(p, len − 1); p ≤ len − 1 for every row below Sq, so the
// length needs no test of its own.
//
// Lanes. i = lane & 15, g = lane >> 4, as in attn_decode.h:
// v_mfma_f32_16x16x32_bf16 takes from lane (i, g) A[row i][k 8g..8g+7] and
// B[k 8g..8g+7][col i] and leaves D[row 4g+r][col i] in accumulator element r.
//
// Scores, Sᵀ = K·Qᵀ. B is Q: lane (i, g) holds for row tile rt and k-step ks
// the 16 bytes at 64ks + 16g of query row 32w + 16rt + i, loaded once per
// block from global memory (2 × 4 fragments, 32 VGPRs); a row at or past Sq
// loads row Sq − 1 (clamped) and is never stored. A is K from LDS: for the 16
// keys of sub-tile t (four per tile) and k-step ks lane (i, g) reads with one
// ds_read_b128 the 16 bytes at 64ks + 16g of tile row 16t + i; each fragment
// feeds the MFMAs of both row tiles. Lane (i, g) ends with the scores of
// query i at keys 64j + 16t + 4g + r: all sixteen values of a row tile in a
// lane belong to one query, so maximum, sum and rescale are per lane and the
// maximum is shared among the lanes i, i+16, i+32, i+48 by two xor-shuffles.
//
// Softmax: decode's, per row tile. scale·log2(e) in fp32 after the MFMA,
// v_exp_f32, rescale only when some lane's maximum moved (wave vote), the
// exponent taken against 0 while the maximum is −inf, P rounded to bf16 (RNE)
// and the running sum fed with the rounded values.
//
// Output, Oᵀ = Vᵀ·Pᵀ. Per 32 keys (half u of the tile) and 16 values of d
// (db = 0..7) one MFMA per row tile. B is Pᵀ: k-slot 8g + 4t' + r is key
// 32u + 16t' + 4g + r, what the lane holds from sub-tile t = 2u + t': four
// v_cvt_pk, no LDS, no cross-lane move. A is Vᵀ, read transposed from LDS with
// ds_read_b64_tr_b16 exactly as in decode (lane j of group g addresses row
// 16t + 4g + j/4, d = 16db + 4(j%4)); one V fragment feeds both row tiles.
// Lane (i, g) ends with Oᵀ[16db + 4g + r][query i]: O/L rounded once to bf16,
// four consecutive d of one row in one 8-byte store.
//
// LDS. 64 KiB: K buffers at 0 and 16 KiB, V buffers at 32 and 48 KiB, a tile
// of 64 rows × 256 bytes each, tile j in buffer j & 1; two blocks per CU. A
// tile is filled by 16 global_load_lds_dwordx4 per operand, four per wave:
// DMA q writes LDS bytes [1024q, +1024), rows 4q .. 4q+3; lane l covers row
// r = 4q + l/16 and physical 16-byte chunk c = l%16. The DMA writes
// lane-linearly, so the swizzle is on the source address. Key rows past
// len − 1 load row len − 1 (clamped, in bounds); their scores are masked.
//   V: chunk c is loaded from logical chunk c ^ 2(r & 7), decode's swizzle,
//   and its argument holds unchanged (the rows of a tile are 0..63 instead of
//   0..31, the reads address the same 16t + 4g + j/4): a b64 read is served
//   in two halves of 32 lanes, a half covers eight rows with eight different
//   r & 7, hence eight different 32-byte blocks, all 64 banks once.
//   K: chunk c is loaded from logical chunk c ^ (r & 15). A ds_read_b128 is
//   served 16 lanes at a time (16 × 16 bytes = all 64 banks once). The 16
//   lanes of group g read logical chunk 4ks + g of rows 16t + i, i = 0..15:
//   unswizzled those are 16 rows 256 bytes apart, the same four banks, 16-way.
//   Swizzled they sit at physical chunks (4ks + g) ^ i, which are sixteen
//   different chunks as i runs, so every bank is touched once.
//
// Schedule and waits. Iteration j: wait for the wave's own DMAs of tile j,
// s_barrier, issue the DMAs of tile j+1 into the other buffers, then the 64
// MFMAs of tile j with their 16 ds_read_b128 and 32 ds_read_b64_tr_b16. One
// barrier per tile: behind it every wave's share of tile j is in LDS, and
// every wave has finished reading tile j−1, whose buffers tile j+1 may then
// overwrite. The DMAs of tile j+1 have the whole of tile j's arithmetic to
// land. The wait is vmcnt(0), and that is a count, not a shortcut: with two
// buffers per operand and one barrier per tile, a buffer is read in every
// other barrier interval, may only be written in the interval between, and
// must be complete at that interval's end because its readers are the other
// waves. So every DMA is issued and retired inside one interval, the wave has
// no other vector memory operation in the loop, and at the wait exactly the 8
// DMAs of tile j are outstanding, all needed. A non-zero count would need a
// third buffer (96 KiB, one block per CU) or a second barrier per tile. The
// block's last tile stages nothing, so no DMA outlives the loop.
// Decode's two findings about the compiler's own vmcnt(0) apply: every LDS
// read here is inline assembly with its own lgkmcnt wait, because given the
// builtin or a plain load the compiler, which cannot tell those reads from the
// DMA writes in flight, drains vmcnt before them and would serialise tile
// j+1's DMA with tile j's arithmetic; and there are no register loads in the
// loop for it to order against the DMAs (Q is loaded before the first wait).
//
// Registers. __launch_bounds__(256, 2): without the second argument the
// compiler spreads over 190 VGPRs + 96 AGPRs, one wave per SIMD, and only one
// block fits a CU; with it 198 VGPRs, no AGPRs, no scratch, two blocks per CU.
//
// Measured on the MI355X (profiles/attn_prefill_ab.md), TFLOP/s over 512 flops
// per visible (query, key) pair and head, kernel plus launch between events,
// gemm_bf16_nt at 8192³ 1344-1361 in the same process: B×Hkv×G, Sq
// 1×8×8, 8192 833-848; 4×8×8, 4096 754-786; 8×8×8, 2048 after 6144 keys of
// context 748-754; a ragged 16×8×8 batch left-padded to 8192 709-714. Per
// tile the block's LDS reads (128 KiB) take as long as a SIMD's 64 MFMAs.

constexpr int AP_THREADS = 256;
constexpr int AP_ROWS = 128;               // query rows per block, 32 per wave
constexpr int AP_TILE = 64;                // keys per tile
constexpr int AP_BUF = AP_TILE * 256;      // one tile of K or V: 16 KiB
constexpr int AP_V0 = 2 * AP_BUF;          // V buffers behind the two K buffers
constexpr int AP_LDS = 4 * AP_BUF;

// K fragments of two sub-tiles (rows OFF/256 .. +31 of a buffer): kf[4t' + ks].
template <int OFF>
__device__ __forceinline__ void ap_read_k(u32x4 (&kf)[8], const uint32_t (&a)[4]) {
  asm volatile(
      "ds_read_b128 %0, %8 offset:%12\n\tds_read_b128 %1, %9 offset:%12\n\t"
      "ds_read_b128 %2, %10 offset:%12\n\tds_read_b128 %3, %11 offset:%12\n\t"
      "ds_read_b128 %4, %8 offset:%13\n\tds_read_b128 %5, %9 offset:%13\n\t"
      "ds_read_b128 %6, %10 offset:%13\n\tds_read_b128 %7, %11 offset:%13\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(kf[0]), "=&v"(kf[1]), "=&v"(kf[2]), "=&v"(kf[3]), "=&v"(kf[4]), "=&v"(kf[5]), "=&v"(kf[6]), "=&v"(kf[7])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(OFF), "n"(OFF + 16 * 256)
      : "memory");
}

// Vᵀ fragments of one 32-key half (rows (OFF − AP_V0)/256 .. +31 of a buffer) for four db: vf[db][t'].
template <int OFF>
__device__ __forceinline__ void ap_read_v(u32x2 (&vf)[4][2], uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:%12\n\tds_read_b64_tr_b16 %1, %8 offset:%13\n\t"
      "ds_read_b64_tr_b16 %2, %9 offset:%12\n\tds_read_b64_tr_b16 %3, %9 offset:%13\n\t"
      "ds_read_b64_tr_b16 %4, %10 offset:%12\n\tds_read_b64_tr_b16 %5, %10 offset:%13\n\t"
      "ds_read_b64_tr_b16 %6, %11 offset:%12\n\tds_read_b64_tr_b16 %7, %11 offset:%13\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(vf[0][0]), "=&v"(vf[0][1]), "=&v"(vf[1][0]), "=&v"(vf[1][1]), "=&v"(vf[2][0]), "=&v"(vf[2][1]),
        "=&v"(vf[3][0]), "=&v"(vf[3][1])
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(OFF), "n"(OFF + 16 * 256)
      : "memory");
}

__global__ __launch_bounds__(AP_THREADS, 2) void attn_prefill(const uint16_t* __restrict__ Q,
                                                          const unsigned char* __restrict__ K,
                                                          const unsigned char* __restrict__ V,
                                                          const int* __restrict__ seq_lens, uint16_t* __restrict__ O,
                                                          int B, int Hkv, int G, int Sq, int s_max, float scale) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15;
  const int g = lane >> 4;
  const int Hq = Hkv * G;

  // Block id, fastest first: head in its group, KV head, sequence, query tile from the last.
  int bid = blockIdx.x;
  const int hg = bid % G;
  bid /= G;
  const int hk = bid % Hkv;
  bid /= Hkv;
  const int b = bid % B;
  const int r0 = ((Sq + AP_ROWS - 1) / AP_ROWS - 1 - bid / B) * AP_ROWS;
  const int h = hk * G + hg;

  const int len = min(max(seq_lens[b], 0), s_max);
  const int last = max(len - 1, 0);  // the row that out-of-range keys load
  const int pos0 = len - Sq;         // position of query row 0; row i sees the keys s <= pos0 + i
  const int p_last = pos0 + min(r0 + AP_ROWS - 1, Sq - 1);
  const int nt = p_last >= 0 ? p_last / AP_TILE + 1 : 0;  // key tiles of the block
  const int wrow = r0 + 32 * wave;                        // the wave's first row
  const int p_wlast = pos0 + min(wrow + 31, Sq - 1);
  const int ntw = wrow < Sq && p_wlast >= 0 ? p_wlast / AP_TILE + 1 : 0;  // tiles this wave computes, <= nt
  const int p_wfirst = pos0 + wrow;
  const uint32_t base = static_cast<uint32_t>(b * Hkv + hk) * static_cast<uint32_t>(s_max) * 256u;
  const float sc = scale * 1.44269504088896340736f;

  // Q fragments and per-lane row state: row tile rt is query row wrow + 16rt + i.
  bf16x8 qf[2][4];
  int row[2], plim[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    row[rt] = wrow + 16 * rt + i;
    plim[rt] = min(pos0 + row[rt], len - 1);
    const uint16_t* qrow = Q + ((static_cast<size_t>(b) * Sq + min(row[rt], Sq - 1)) * Hq + h) * 128 + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[rt][ks] = *reinterpret_cast<const bf16x8*>(qrow + 32 * ks);
  }

  // This wave's share of tile j: DMAs 4·wave .. 4·wave+3 of K and of V, tile rows 16·wave .. +15.
  auto stage = [&](int buf, int j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = 4 * q + g;  // tile row 16·wave + x of lane l = 16g + i, physical chunk i
      const uint32_t src = base + static_cast<uint32_t>(min(j * AP_TILE + 16 * wave + x, last)) * 256u;
      unsigned char* dst = smem + buf * AP_BUF + (4 * wave + q) * 1024;
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(K + src + ((i ^ x) << 4)),
                                       (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(V + src + ((i ^ ((x & 7) << 1)) << 4)),
                                       (__attribute__((address_space(3))) void*)(dst + AP_V0), 16, 0, 0);
    }
  };

  const uint32_t lds0 =
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)(smem)));
  uint32_t k_addr[4];  // row i of sub-tile 0 of K buffer 0, logical chunk 4ks + g at physical (4ks + g) ^ i
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) k_addr[ks] = lds0 + i * 256 + (((4 * ks + g) ^ i) << 4);
  // Transposing reads: lane j = i of group g addresses row 16t + 4g + j/4, bytes 32·(db ^ (row & 7)) + 8(j%4).
  const int rd_row = 4 * g + (i >> 2);
  uint32_t v_addr[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) v_addr[db] = lds0 + rd_row * 256 + ((db ^ (rd_row & 7)) << 5) + ((i & 3) << 3);

  float m[2] = {AD_NEG_INF, AD_NEG_INF}, l[2] = {0.f, 0.f};
  f32x4 acc[2][8];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int db = 0; db < 8; ++db) acc[rt][db] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto step = [&](auto slot_c, int j) {
    constexpr int slot = decltype(slot_c)::value;
    // The 8 DMAs of tile j are this wave's only vector memory operations in flight (header: Schedule and waits).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (j + 1 < nt) stage(slot ^ 1, j + 1);
    __builtin_amdgcn_sched_barrier(0);
    if (j >= ntw) return;
    const int kv0 = j * AP_TILE;

    f32x4 s[2][4];  // [rt][t]
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 4; ++t) s[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto scores = [&](auto pair_c) {
      constexpr int pair = decltype(pair_c)::value;  // sub-tiles 2·pair and 2·pair + 1
      u32x4 kf[8];
      ap_read_k<slot * AP_BUF + pair * 32 * 256>(kf, k_addr);
#pragma unroll
      for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
            s[rt][2 * pair + tp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, kf[4 * tp + ks]), qf[rt][ks], s[rt][2 * pair + tp], 0, 0, 0);
    };
    scores(std::integral_constant<int, 0>{});
    scores(std::integral_constant<int, 1>{});
    __builtin_amdgcn_sched_barrier(0);

    const bool diagonal = kv0 + AP_TILE - 1 > p_wfirst;  // some (row, key) of this wave's 32 × 64 is masked
    uint32_t pk[2][8];                                    // [rt][2t + half]: P as bf16 pairs
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float mt = AD_NEG_INF;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = s[rt][t][r] * sc;
          s[rt][t][r] = !diagonal || kv0 + 16 * t + 4 * g + r <= plim[rt] ? v : AD_NEG_INF;
          mt = fmaxf(mt, s[rt][t][r]);
        }
      mt = fmaxf(mt, __shfl_xor(mt, 16));
      mt = fmaxf(mt, __shfl_xor(mt, 32));
      const float m_new = fmaxf(m[rt], mt);
      const float m_ref = m_new == AD_NEG_INF ? 0.f : m_new;  // nothing seen yet: exp2(−inf − 0) = 0
      if (__any(m_new > m[rt])) {
        const float alpha = m_new > m[rt] ? __builtin_amdgcn_exp2f(m[rt] - m_ref) : 1.f;
        l[rt] *= alpha;
#pragma unroll
        for (int db = 0; db < 8; ++db) acc[rt][db] *= alpha;
      }
      m[rt] = m_new;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const uint32_t u = pack_bf16x2(__builtin_amdgcn_exp2f(s[rt][t][2 * hf] - m_ref),
                                         __builtin_amdgcn_exp2f(s[rt][t][2 * hf + 1] - m_ref));
          pk[rt][2 * t + hf] = u;
          l[rt] += __builtin_bit_cast(float, u << 16) + __builtin_bit_cast(float, u & 0xffff0000u);
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    auto output = [&](auto half_c) {
      constexpr int u = decltype(half_c)::value;  // keys 32u .. 32u+31 of the tile
      bf16x8 pf[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
        pf[rt] = __builtin_bit_cast(bf16x8, (u32x4){pk[rt][4 * u], pk[rt][4 * u + 1], pk[rt][4 * u + 2], pk[rt][4 * u + 3]});
#pragma unroll
      for (int hb = 0; hb < 8; hb += 4) {
        u32x2 vf[4][2];  // [db − hb][t']
        ap_read_v<AP_V0 + slot * AP_BUF + u * 32 * 256>(vf, v_addr[hb], v_addr[hb + 1], v_addr[hb + 2], v_addr[hb + 3]);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const bf16x8 vt = __builtin_bit_cast(bf16x8, (u32x4){vf[d][0][0], vf[d][0][1], vf[d][1][0], vf[d][1][1]});
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
            acc[rt][hb + d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt, pf[rt], acc[rt][hb + d], 0, 0, 0);
        }
      }
    };
    output(std::integral_constant<int, 0>{});
    output(std::integral_constant<int, 1>{});
    __builtin_amdgcn_sched_barrier(0);
  };

  if (nt > 0) {
    stage(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    for (int j = 0; j < nt; j += 2) {
      step(std::integral_constant<int, 0>{}, j);
      if (j + 1 >= nt) break;
      step(std::integral_constant<int, 1>{}, j + 1);
    }
  }

  // O/L, once to bf16; a row that saw no key (L = 0) stores 0, a row at or past Sq stores nothing.
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float L = l[rt];
    L += __shfl_xor(L, 16);
    L += __shfl_xor(L, 32);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    if (row[rt] >= Sq) continue;
    uint16_t* orow = O + ((static_cast<size_t>(b) * Sq + row[rt]) * Hq + h) * 128 + 4 * g;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const f32x4 o = acc[rt][db] * inv;
      *reinterpret_cast<u32x2*>(orow + 16 * db) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
    }
  }
}

bool g_attn_prefill_attr = false;

const char* launch_attn_prefill(const void* q, const void* k, const void* v, const void* lens, void* out, int b, int hkv,
                                int g, int sq, int s_max, float scale, hipStream_t stream) {
  if (b < 1 || b > 65535 || hkv < 1 || g < 1 || sq < 1 || s_max < 1)
    return "attn_prefill_bf16: needs 1 <= B <= 65535, Hkv >= 1, Hq/Hkv >= 1, Sq >= 1, S_max >= 1";
  if (static_cast<uint64_t>(b) * hkv * s_max * 256 >= (1ull << 32))
    return "attn_prefill_bf16: a cache must be smaller than 2^32 bytes (B*Hkv*S_max*256)";
  if (static_cast<uint64_t>(b) * sq * 256 * hkv * g >= (1ull << 32))
    return "attn_prefill_bf16: q must be smaller than 2^32 bytes (B*Sq*Hq*256)";
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return "attn_prefill_bf16: q, k_cache, v_cache and out must be 16-byte aligned";
  if (lens == nullptr || (reinterpret_cast<uintptr_t>(lens) & 3)) return "attn_prefill_bf16: seq_lens must be 4-byte aligned";
  if (!g_attn_prefill_attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(attn_prefill), hipFuncAttributeMaxDynamicSharedMemorySize,
                            AP_LDS) != hipSuccess)
      return "attn_prefill_bf16: cannot reserve LDS";
    g_attn_prefill_attr = true;
  }
  // B·Hq·⌈Sq/128⌉ <= B·Hq·Sq < 2^24 by the limit on q above.
  const unsigned blocks = static_cast<unsigned>(b) * hkv * g * ((sq + AP_ROWS - 1) / AP_ROWS);
  hipLaunchKernelGGL(attn_prefill, dim3(blocks), dim3(AP_THREADS), AP_LDS, stream, static_cast<const uint16_t*>(q),
                     static_cast<const unsigned char*>(k), static_cast<const unsigned char*>(v),
                     static_cast<const int*>(lens), static_cast<uint16_t*>(out), b, hkv, g, sq, s_max, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

PyObject* py_attn_prefill(PyObject*, PyObject* args) {
  unsigned long long q, k, v, lens, out, stream;
  int b, hkv, g, sq, s_max;
  double scale;
  if (!PyArg_ParseTuple(args, "KKKKKiiiiidK", &q, &k, &v, &lens, &out, &b, &hkv, &g, &sq, &s_max, &scale, &stream))
    return nullptr;
  const char* err = launch_attn_prefill(reinterpret_cast<void*>(q), reinterpret_cast<void*>(k),
                                        reinterpret_cast<void*>(v), reinterpret_cast<void*>(lens),
                                        reinterpret_cast<void*>(out), b, hkv, g, sq, s_max, static_cast<float>(scale),
                                        reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

constexpr const char* kAttnPrefillDoc =
    "attn_prefill_bf16(q, k_cache, v_cache, seq_lens, out, B, Hkv, G, Sq, S_max, scale, stream): causal "
    "softmax(scale q k^T) v of Sq query rows per sequence, q and out [B,Sq,Hq,128], over a bf16 KV cache "
    "[B,Hkv,S_max,128], Hq = G*Hkv; query row i sits at position seq_lens[b] - Sq + i and sees the keys up to it.";
