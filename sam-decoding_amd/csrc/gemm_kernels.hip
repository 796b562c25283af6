// gemm_kernels.hip -- weight-streaming skinny GEMM of the verify forward for gfx950:  out[m][n] = sum_k A[m][k] * W[n][k]
// with m <= 64 draft rows, W = an HF nn.Linear weight [N, K], re-tiled once at load time (samd_gemm_pack_weights) so that
// every workgroup reads its share as one linear stream of 64 KiB blocks.
//
// At <= 64 rows the verify forward is bound by reading the weights once (13.5 GB for Vicuna-7B): the kernel is a weight
// STREAM with a little MFMA attached.  What shapes it (scripts/hbm_probe.hip, scripts/stream_probe.hip, profiles/):
//   * the memory system retires ~48 G requests/s whatever their size, so every request carries full lines: a lane loads
//     16 bytes, a wave-instruction 1 KiB contiguous;
//   * PACKED LAYOUT: block (tile t = 128 output columns, chunk c = 256 k) is 64 KiB contiguous at
//     ((t * K/256 + c) * 4096) uint4 units; inside it unit (2b + j) * 512 + tid holds
//     W[128 t + 16 w + n][256 c + 64 b + 16 g + 8 j .. +7] for tid = 64 w + 16 g + n -- exactly the order the lanes consume
//     (lane (g, n) of wave w feeds column 16 w + n; its 8-element vectors cover k = 64 b + 16 g + 8 j .. within each 64-wide
//     k block, and the A operand is read from LDS with the same k permutation, so the product is unchanged).  Reading the
//     same bytes with this grid from the row-major matrix is 8-9 % slower (79.6 vs 72.8 us for a layer's four projections);
//   * A (the activations, <= 1 MB, L2 resident) is staged per workgroup through LDS by LDS-DMA in 256-wide k chunks, three
//     buffers; the weights go HBM -> VGPR -> MFMA with TWO chunks in flight (see the pipeline comment in the kernel);
//   * one balanced wave of workgroups per launch (samd_gemm_splits); split-K partial sums are written as fp32 and added up
//     by the consuming kernel (rmsnorm + residual, rope), so a split costs no extra launch.
//   * the weight loads carry the nt (non-temporal) policy bit: -10 % on every projection launch (round 2; an earlier test through
//     __builtin_nontemporal_load on the pre-asm kernel had shown nothing);
// Measured and dropped: a 16-row variant that stages the whole A slice once (159 vs 141 us per layer),
// 16-wave workgroups, an intra-workgroup K split, an Infinity-Cache warmer on a side stream, producers of A inside the launch
// (DESIGN.md, K7).  Ablation: with the MFMAs and the LDS traffic compiled out the kernel is 3 % faster -- it runs at what
// separate launches of 33-180 MB can stream (4.1-5.9 TB/s incl. ramp-up and tail).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "samd_common.h"

#define LAUNCHCHK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { samd_set_error("kernel launch: %s", hipGetErrorString(e_)); return SAMD_E_HIP; } } while (0)

static int samd_cu_count() { return samd_device_cus(); }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct GF16 { typedef _Float16 elem; typedef half8 vec8;
    static __device__ __forceinline__ floatx4 mfma(half8 a, half8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); } };
struct GBF16 { typedef __bf16 elem; typedef bf16x8 vec8;
    static __device__ __forceinline__ floatx4 mfma(bf16x8 a, bf16x8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); } };

#define GEMM_KC 256                    // k elements per chunk
#define GEMM_WAVES 8                   // waves per workgroup; each wave owns 16 output columns
#define GEMM_COLS (16 * GEMM_WAVES)    // output columns per workgroup

typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

// Diagnostic build only (-DSAMD_GEMM_ABLATE, scripts/r05_ablate.sh; never in the shipped library): k_gemm_pairs_silu with parts switched off at
// run time by SAMD_GEMM_ABL -- bit 0: no s_barrier per chunk (results wrong, timing only), bit 1: no LDS reads / MFMAs, bit 2: no A staging,
// bit 3: A fetched from rows 0..15 only (L1 hits instead of L2 traffic) -- to see where the 64-row tile loses its time (profiles/r05_wide_tile.md)
#ifdef SAMD_GEMM_ABLATE
__device__ int samd_abl_flag;
#endif

// EPI 0: out / fp32 partials as they are.  EPI 1 (splits == 1 only): the matrix is the MLP's gate|up pair with its rows
// interleaved in groups of 64 (tile t = gate columns 64t.. | up columns 64t..), and the epilogue writes
// silu(gate) * up [rows][N/2] -- LlamaMLP's activation without a launch, a 2N-wide intermediate or its re-read.
// DEPTH = weight chunks (+ their A tiles) in flight whenever a wave waits; DEPTH + 1 LDS buffers (dynamic LDS: 128 KiB at 64 rows).
// GM (round 6): W is GROUP-MAJOR (samd_gemm_pack_groups: column group gi = 16 columns, chunk c = 8 KiB contiguous at (gi * K/256 + c) * 512 units,
// unit (2b + j) * 64 + lane -- the layout k_gemm_cs_residual and k_gemm_pairs_silu stream) instead of 128-column tiles: wave w of tile t reads
// group 8 t + w as its own 1 KiB-per-instruction stream.  o_proj / down_proj then need ONE packed copy for every row bucket (the complete-sum
// kernels of <= 16 rows and this split-K kernel above them) instead of two: -4 GB of a 7B replica.
template <typename TT, int RT, int EPI, int DEPTH, bool GM = false>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT >= 3 || DEPTH > 2 ? 2 : GEMM_WAVES / 2) void k_gemm_skinny(const typename TT::elem *__restrict__ A, const typename TT::elem *__restrict__ W,
                                                        float *__restrict__ partial, typename TT::elem *__restrict__ out,
                                                        int K, int N, int n_chunks, int n_splits) {
    typedef typename TT::elem E;
    typedef typename TT::vec8 V8;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk (R rows x 32 units)
    // A tile: [R rows][32 units of 16 B], unit u of row r stored at position u ^ (r & 15): the 16 rows that one
    // ds_read_b128 wave-instruction touches (same unit, rows m..m+15) land in 16 different 16-byte slots -> no bank
    // conflict, and rows stay contiguous so the tile can be filled by LDS-DMA (global_load_lds, 1 KiB per wave-instruction,
    // no VGPR round trip; the swizzle goes on the SOURCE address).
    constexpr int NB = DEPTH + 1;
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    const int n0 = blockIdx.x * GEMM_COLS + 16 * w;
    const int split = blockIdx.y;
    const int c0 = (int)((long long)split * n_chunks / n_splits), c1 = (int)((long long)(split + 1) * n_chunks / n_splits);
    constexpr size_t WCH = GM ? 8192 : 65536, WU = GM ? 1024 : 8192;      // bytes of one (stream, chunk) block; of one (b, j) unit row inside it
    const int ws = GM ? __builtin_amdgcn_readfirstlane(GEMM_WAVES * (int)blockIdx.x + w) : (int)blockIdx.x;      // this wave's stream: its group / the tile
    const char *wtile = reinterpret_cast<const char *>(W) + (size_t)ws * n_chunks * WCH;           // packed: see header
    const uint32_t wlane = (uint32_t)(GM ? l : tid) * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    // The weight loads, the LDS reads and the waits between them are hand-issued.  The compiler's wait-count pass is
    // path-insensitive and cannot tell which LDS buffer an LDS-DMA in flight writes: left to itself it drains every
    // outstanding load (vmcnt(0)) in front of each chunk's first LDS read and first MFMA, which leaves ONE chunk in flight.
    // Here TWO chunks (+ their A tiles) are in flight whenever a wave waits: memory ops retire in issue order, so "chunk c
    // has landed, chunk c+1 may still fly" is vmcnt(8 + XV).  scripts/stream_probe.hip: 18.3 vs 20.2 us for the QKV matrix.
    u32x4 wr[DEPTH][4][2];
    auto load_wb = [&](u32x4 (&dst)[4][2], int c, int b) {
        const char *p = wtile + (size_t)c * WCH;                     // wave-uniform -> SGPR base, one offset VGPR
#pragma unroll
        for (int j = 0; j < 2; j++)        // nt: every weight byte is read once, by one CU -- streamed past the caches (13.7 vs 15.1 us, 30.1 vs 33.3)
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst[b][j]) : "v"(wlane), "s"(p + WU * (2 * b + j)) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {   // asynchronous: lands in LDS, counted by vmcnt
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)row * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;       // wave-uniform base; the hardware adds lane * 16 B
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4][2], int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    // wait for the oldest chunk in flight, then meet the other waves -- their LDS-DMA shares of the A tile are then in
    // place.  Bare s_barrier: __syncthreads() carries a fence that would drain the younger chunk as well.  Nothing ties
    // the weight registers to the wait (an in/out operand would make the compiler copy them BEFORE the wait, i.e. while
    // the load is in flight); instead every MFMA also consumes an LDS operand that a volatile asm after the wait produces,
    // and volatile asm statements keep their order.
    auto landed = [&](int younger_in_flight) {
        if (DEPTH > 2 && younger_in_flight >= 2) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * (8 + XV)) : "memory");
        else if (younger_in_flight >= 1) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(8 + XV) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // one phase: MFMAs of chunk c out of `cur` / LDS buffer `buf`, then the same registers are refilled with chunk c + DEPTH
    // and LDS buffer (buf - 1) mod NB, which every wave finished reading before this phase's barrier
    auto phase = [&](u32x4 (&cur)[4][2], int c, int buf) {
        landed(c1 - 1 - c);
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t u0 = (uint32_t)((8 * b + 2 * g) ^ n) * 16, u1 = (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;   // rows 16 mt + n: (row & 15) == n
            // all row tiles of this k block in one LDS round trip (row tile mt sits 16 rows = 8 KiB further: immediate offsets)
            const uint32_t a0 = xbase + u0, a1 = xbase + u1;
            u32x4 r[RT][2];
            if constexpr (RT == 1)
                asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]) : "v"(a0), "v"(a1));
            else if constexpr (RT == 2)
                asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %4 offset:8192\n\tds_read_b128 %3, %5 offset:8192\n\t"
                             "s_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]) : "v"(a0), "v"(a1));
            else if constexpr (RT == 3)
                asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %6 offset:8192\n\tds_read_b128 %3, %7 offset:8192\n\t"
                             "ds_read_b128 %4, %6 offset:16384\n\tds_read_b128 %5, %7 offset:16384\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]) : "v"(a0), "v"(a1));
            else
                asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %8 offset:8192\n\tds_read_b128 %3, %9 offset:8192\n\t"
                             "ds_read_b128 %4, %8 offset:16384\n\tds_read_b128 %5, %9 offset:16384\n\tds_read_b128 %6, %8 offset:24576\n\t"
                             "ds_read_b128 %7, %9 offset:24576\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]), "=&v"(r[3][0]), "=&v"(r[3][1])
                             : "v"(a0), "v"(a1));
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][0]), __builtin_bit_cast(V8, cur[b][0]), acc[mt]);
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][1]), __builtin_bit_cast(V8, cur[b][1]), acc[mt]);
            }
            // 64 rows: refill as soon as this k block's operands are consumed -- the loads trickle into the memory pipe between
            // the k blocks instead of arriving as one burst after a load-free compute window (all 8 waves compute at once):
            // gate|up 40.5 -> 39.8 us; neutral at 16 / 32 rows, which keep the burst (profiles/r02_gemm_rows64.md)
            if (RT >= 3 && c + DEPTH < c1) {
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
            }
        }
        if (RT < 3 && c + DEPTH < c1) { load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
    if (c0 < c1) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c0 + d < c1) { load_w(wr[d], c0 + d); stage_x(c0 + d, d); }
        int buf = 0;
        for (int c = c0; c < c1; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < c1) { phase(wr[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // C layout of mfma_16x16: lane holds rows 4g + r of column n
    if constexpr (EPI == 1) {
        float *ex = reinterpret_cast<float *>(gemm_lds);            // [R][64] up values; the A tiles are dead by now
        __syncthreads();
        if (w >= 4) {
#pragma unroll
            for (int mt = 0; mt < RT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) ex[(16 * mt + 4 * g + r) * 64 + 16 * (w - 4) + n] = acc[mt][r];
        }
        __syncthreads();
        if (w < 4) {
#pragma unroll
            for (int mt = 0; mt < RT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int m = 16 * mt + 4 * g + r;
                    // the roundings of HF's act_fn(gate_proj(x)) * up_proj(x) in the model dtype (same as k_silu_mul)
                    const float gf = (float)(E)acc[mt][r], uf = (float)(E)ex[m * 64 + 16 * w + n];
                    const E sv = (E)(gf / (1.f + __expf(-gf)));
                    out[(size_t)m * (N / 2) + blockIdx.x * 64 + 16 * w + n] = (E)((float)sv * uf);
                }
        }
        return;
    }
#pragma unroll
    for (int mt = 0; mt < RT; mt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 16 * mt + 4 * g + r;
            if (out) out[(size_t)m * N + n0 + n] = (E)acc[mt][r];
            // write-through (sc1) stores: the fp32 partials leave the L2 while the launch still streams, instead of as dirty lines the
            // kernel boundary has to flush (64 rows: 46 MB per layer; 3.93 -> 3.89 ms per step, neutral at 16 rows)
            else __hip_atomic_store(&partial[((size_t)split * R + m) * N + n0 + n], acc[mt][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// RMSNorm applied by the CONSUMING projection (NORM variants of k_gemm_qkv_rope / k_gemm_pairs_silu): the rows' sums of squares arrive as
// per-16-column partials (k_gemm_cs_residual, k_embed_rows_ssq), every workgroup adds them up in the same fixed order and keeps
// 1 / rms per row in LDS; the A chunks then pass through registers instead of the LDS DMA and are scaled there with the reference's
// roundings: h = (x * rsqrt(mean(x^2) + eps)).to(dtype), a = weight * h (LlamaRMSNorm.forward).
struct NormArgs { const float *ssq; const void *g; int tiles; float inv_hidden; float eps; };

// the partial sums are REQUESTED before the first weight chunks (hand-issued loads, so that the counted waits of the stream stay exact) and
// added up once those chunks are in flight: up to NORM_NS loads per thread (rounds past the tile count are skipped, the last one is clamped + zeroed)
#define NORM_NS 16
template <int NT>
__device__ __forceinline__ void norm_issue(const NormArgs &na, float (&sv)[NORM_NS]) {
    const int tid = threadIdx.x, row = tid & 15, p = tid >> 4;
#pragma unroll
    for (int k = 0; k < NORM_NS; k++) {
        sv[k] = 0.f;
        if ((NT / 16) * k >= na.tiles) continue;             // (uniform) nothing of this round exists: K = 4096 needs 8 of the 16 rounds
        int t = p + (NT / 16) * k;
        t = t < na.tiles ? t : na.tiles - 1;
        const float *src = na.ssq + (size_t)t * 16 + row;
        asm volatile("global_load_dword %0, %1, off" : "=v"(sv[k]) : "v"(src) : "memory");
    }
}
template <int NT>
__device__ __forceinline__ void norm_finish(const NormArgs &na, float (&sv)[NORM_NS], float *part /* [NT / 16][16] */, float *rs /* [16] */) {
    const int tid = threadIdx.x, row = tid & 15, p = tid >> 4;
    // the caller's counted wait has just retired the loads of norm_issue.  The compiler does not know that those asm statements were
    // asynchronous: this statement re-defines their destinations HERE, so that no use can be scheduled above the wait and the registers
    // stay reserved until it (without it a build with branches around the loads consumed a register one instruction after its load was
    // issued and recycled it as an address while the load was in flight)
    static_assert(NORM_NS == 16, "");
    asm volatile("" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(sv[4]), "+v"(sv[5]), "+v"(sv[6]), "+v"(sv[7]),
                      "+v"(sv[8]), "+v"(sv[9]), "+v"(sv[10]), "+v"(sv[11]), "+v"(sv[12]), "+v"(sv[13]), "+v"(sv[14]), "+v"(sv[15]) : : "memory");
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NORM_NS; k++) s += (p + (NT / 16) * k < na.tiles) ? sv[k] : 0.f;
    part[p * 16 + row] = s;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (tid < 16) {
        float tot = 0.f;
        for (int k = 0; k < NT / 16; k++) tot += part[k * 16 + tid];
        rs[tid] = rsqrtf(tot * na.inv_hidden + na.eps);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <typename E>
__device__ __forceinline__ u32x4 norm_scale8(u32x4 xraw, u32x4 graw, float rs) {
    const E *xe = reinterpret_cast<const E *>(&xraw);
    const E *ge = reinterpret_cast<const E *>(&graw);
    u32x4 out;
    E *oe = reinterpret_cast<E *>(&out);
#pragma unroll
    for (int j = 0; j < 8; j++) { const E h = (E)((float)xe[j] * rs); oe[j] = (E)((float)ge[j] * (float)h); }
    return out;
}

// one staged unit of an ODD row count (AR rows of 32 lanes each): the x and g loads under a wave-uniform lane mask.  The wave ISSUES both
// loads whatever the mask, so the counted waits stay exact; a masked-off lane fetches nothing and keeps stale registers.  One statement
// with unconditional outputs, not a branch around the loads: the compiler must see no path on which it may copy a register in flight
__device__ __forceinline__ void norm_load_masked(u32x4 &xd, u32x4 &gd, const void *xsrc, const void *gsrc, unsigned long long mask) {
    unsigned long long saved;
    asm volatile("s_and_saveexec_b64 %2, %5\n\tglobal_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %4, off\n\ts_mov_b64 exec, %2"
                 : "=&v"(xd), "=&v"(gd), "=&s"(saved) : "v"(xsrc), "v"(gsrc), "s"(mask) : "memory", "scc");
}

// counted wait of the weight stream: memory operations retire in issue order, so chunk c has landed when at most `younger` x PC
// operations (PC = this wave's memory operations per chunk) may still fly
template <int DEPTH, int PC>
__device__ __forceinline__ void gemm_wait_younger(int younger) {
    if constexpr (PC == 0) asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    else {
        if (DEPTH > 3 && younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(3 * PC) : "memory");
        else if (DEPTH > 2 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * PC) : "memory");
        else if (younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(PC) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    }
}

// ================================================================================================
// q|k|v projection with RoPE and the K/V row write as its epilogue (round 3): the k_rope_kv launch and the fp32 split-K partials of the
// q|k|v projection disappear (Vicuna-7B: 5 us and 1.5 MB written + read back per layer).  An epilogue needs COMPLETE sums, so no split-K
// across workgroups: the launch gets its workgroups from 64-column tiles instead -- (H + 2 H_kv) x 2 of them, 192 for a 32-head MHA
// model -- and the two halves of every 256-k chunk go to two wave groups of the same workgroup (waves 0-3: k blocks 0,1; waves 4-7:
// k blocks 2,3; 16 columns each), whose accumulators meet in LDS after the stream.  A tile holds 32 complete rotate_half PAIRS of one
// head -- head columns {32 half + i, 64 + 32 half + i : i < 32} -- so the rotation needs nothing from another workgroup; the row
// permutation is applied once, when the weights are packed (samd_gemm_pack_qkv64).
//   PACKED LAYOUT (64-column tiles): block (tile t, chunk c) = 32 KiB contiguous at ((t * K/256 + c) * 2048) uint4 units; unit
//   (2 bl + j) * 512 + tid holds Wperm[64 t + 16 cg + n][256 c + 64 (2 kh + bl) + 16 g + 8 j .. +7] for tid = 64 (4 kh + cg) + 16 g + n.
// The stream itself is k_gemm_skinny's: LDS-DMA'd A chunks shared by all waves, hand-issued nt weight loads with DEPTH chunks in flight
// (32 KiB chunks: DEPTH 4 = the same 128 KiB per workgroup), counted waits, bare barriers.
// ================================================================================================
// AR (NORM only; round 4): activation rows a workgroup fetches -- 16, or 8 for a draft of <= 8 nodes: waves 0-3 stage rows 0-7, waves 4-7
// stage nothing (rows 8-15 of the LDS tiles are zeroed once), a sixth less of what the CU's memory pipe ingests beside the weights.
// Any AR in 1..16 (the draft's own node count, known on the host): threads 0 .. 32 AR - 1 stage, the others zero rows AR..15 once; with an
// odd AR the upper half of the last staging wave is masked off inside the loads, which the wave still issues (norm_load_masked)
template <typename TT, int RT, int DEPTH, int CG, bool NORM, int AR = 16>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT >= 3 || NORM ? 2 : GEMM_WAVES / 2) void k_gemm_qkv_rope(
        const typename TT::elem *__restrict__ A, const typename TT::elem *__restrict__ W, int K, int n_chunks,
        const float *__restrict__ cs, const int *__restrict__ d_L, const int *__restrict__ d_n,
        typename TT::elem *__restrict__ q_out, typename TT::elem *__restrict__ k_cache, typename TT::elem *__restrict__ v_cache,
        int H, int Hkv, long long max_len, NormArgs na, int v_t) {
    typedef typename TT::elem E;
    typedef typename TT::vec8 V8;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk
    constexpr int NB = DEPTH + 1;
    constexpr int WL = 4;                          // weight loads per lane and chunk (streaming waves)
    constexpr int TW = 16 * CG, PP = 8 * CG;       // tile width in columns, rotate_half pairs per tile
    constexpr int CH = CG * 8192;                  // bytes of one (tile, chunk) block
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    // waves 0 .. 2 CG - 1 stream and multiply (column group cg, k half kh); with 48-column tiles waves 6, 7 only help staging A
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    const bool streams = CG == 4 || w < 2 * CG;
    static_assert(AR == 16 || (AR >= 1 && AR < 16 && NORM && RT == 1), "fewer than 16 activation rows: the norm-fold kernels only");
    const bool stager = AR == 16 || w < (AR + 1) / 2;                            // wave-uniform: a wave with a staging lane (rows 0..AR-1 belong to threads 0..32 AR - 1)
    const bool stages = !(AR & 1) ? stager : tid < 32 * AR;                      // per lane: not the upper half of an odd AR's last staging wave
    const unsigned long long stage_mask = (AR & 1) && __builtin_amdgcn_readfirstlane(w) == AR / 2 ? 0xffffffffull : ~0ull;
    const int cg = CG == 4 ? (w & 3) : (streams ? w % CG : 0), kh = CG == 4 ? (w >> 2) : (streams ? w / CG : 0);
    const char *wtile = reinterpret_cast<const char *>(W) + (size_t)blockIdx.x * n_chunks * CH;
    const uint32_t wlane = (uint32_t)(64 * (CG * kh + cg) + l) * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];
    // the scalars and this thread's cos | sin are requested now and used after the stream
    const int n_rows = d_n[0], L = d_L[0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    u32x4 wr[DEPTH][2][2];
    auto load_wb = [&](u32x4 (&dst)[2][2], int c, int bl) {
        const char *p = wtile + (size_t)c * CH;
#pragma unroll
        for (int j = 0; j < 2; j++)
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst[bl][j]) : "v"(wlane), "s"(p + (CH / 4) * (2 * bl + j)) : "memory");
    };
    // NORM: the A chunk and the norm weights of its k range come through registers (two loads per unit) and are scaled on their way to LDS
    static_assert(!NORM || RT == 1, "the norm-fold path is built for the 16-row tile");
    constexpr int XL = NORM ? 2 * XV : XV;         // memory operations per thread to stage one A chunk
    u32x4 xr[NORM ? DEPTH : 1][NORM ? XV : 1], gr[NORM ? DEPTH : 1][NORM ? XV : 1];
    __shared__ float norm_part[NORM ? (NT / 16) * 16 : 1], norm_rs[NORM ? 16 : 1];
    auto stage_xi = [&](int c, int buf, int i, int d) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)row * K + (size_t)c * GEMM_KC + 8 * unit;
        if constexpr (NORM) {
            const E *gsrc = reinterpret_cast<const E *>(na.g) + (size_t)c * GEMM_KC + 8 * unit;
            if constexpr (AR & 1) norm_load_masked(xr[d][i], gr[d][i], src, gsrc, stage_mask);
            else {
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xr[d][i]) : "v"(src) : "memory");
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gr[d][i]) : "v"(gsrc) : "memory");
            }
        } else {
            E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
            asm volatile("" ::: "memory");
        }
    };
    auto issue = [&](u32x4 (&dst)[2][2], int c, int buf, int d) {
        if (streams) { load_wb(dst, c, 0); load_wb(dst, c, 1); }
        if (stager) {
#pragma unroll
            for (int i = 0; i < XV; i++) stage_xi(c, buf, i, d);
        }
    };
    auto scale_to_lds = [&](int buf, int d) {      // NORM: this thread's units of the landed chunk -> LDS, scaled (same positions as the DMA's)
        if constexpr (NORM) {
            if (!stager) return;
#pragma unroll
            for (int i = 0; i < XV; i++) {
                const int slot = tid + NT * i, row = slot >> 5;
                // (re-defined here, behind the counted wait: the compiler does not know that the asm loads that produced them were asynchronous)
                asm volatile("" : "+v"(xr[d][i]), "+v"(gr[d][i]) : : "memory");
                const u32x4 v = norm_scale8<E>(xr[d][i], gr[d][i], norm_rs[row]);
                if (stages) *reinterpret_cast<u32x4 *>(&xs[buf][0][0] + (size_t)slot * 8) = v;
            }
        }
    };
    auto landed = [&](int younger, int buf, int d) {   // memory ops retire in issue order: chunk c has landed when only the younger ones may still fly
        if (streams) { if (stager) gemm_wait_younger<DEPTH, WL + XL>(younger); else gemm_wait_younger<DEPTH, WL>(younger); }
        else { if (stager) gemm_wait_younger<DEPTH, XL>(younger); else gemm_wait_younger<DEPTH, 0>(younger); }   // (a staging-only / an idle wave)
        if constexpr (NORM) { scale_to_lds(buf, d); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto phase = [&](u32x4 (&cur)[2][2], int c, int buf, int d) {
        landed(n_chunks - 1 - c, buf, d);
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
        for (int bl = 0; bl < 2; bl++) {
            if (!streams) break;
            const int b = 2 * kh + bl;
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            if constexpr (RT == 1)
                asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]) : "v"(a0), "v"(a1));
            else if constexpr (RT == 2)
                asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %4 offset:8192\n\tds_read_b128 %3, %5 offset:8192\n\t"
                             "s_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]) : "v"(a0), "v"(a1));
            else if constexpr (RT == 3)
                asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %6 offset:8192\n\tds_read_b128 %3, %7 offset:8192\n\t"
                             "ds_read_b128 %4, %6 offset:16384\n\tds_read_b128 %5, %7 offset:16384\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]) : "v"(a0), "v"(a1));
            else
                asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %8 offset:8192\n\tds_read_b128 %3, %9 offset:8192\n\t"
                             "ds_read_b128 %4, %8 offset:16384\n\tds_read_b128 %5, %9 offset:16384\n\tds_read_b128 %6, %8 offset:24576\n\t"
                             "ds_read_b128 %7, %9 offset:24576\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]), "=&v"(r[3][0]), "=&v"(r[3][1])
                             : "v"(a0), "v"(a1));
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][0]), __builtin_bit_cast(V8, cur[bl][0]), acc[mt]);
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][1]), __builtin_bit_cast(V8, cur[bl][1]), acc[mt]);
            }
        }
        if (c + DEPTH < n_chunks) issue(cur, c + DEPTH, buf == 0 ? NB - 1 : buf - 1, d);
    };
    float norm_sv[NORM ? NORM_NS : 1];
    if constexpr (NORM) norm_issue<NT>(na, norm_sv);
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if (d < n_chunks) issue(wr[d], d, d, d);
    if constexpr (AR < 16) {                        // rows AR..15 of every A buffer: zero, once (the lanes that stage nothing write them)
        if (!stages) {
#pragma unroll
            for (int bz = 0; bz < NB; bz++) *reinterpret_cast<u32x4 *>(&xs[bz][0][0] + (size_t)tid * 8) = (u32x4){0u, 0u, 0u, 0u};
        }
    }
    if constexpr (NORM) {                           // the partial sums were requested before the chunks: they have landed when only the chunks' operations fly
        if (n_chunks >= DEPTH) {
            if (streams) { if (stager) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * (WL + XL)) : "memory"); else asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * WL) : "memory"); }
            else { if (stager) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * XL) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); }
        } else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        norm_finish<NT>(na, norm_sv, norm_part, norm_rs);
    }
    {
        int buf = 0;
        for (int c = 0; c < n_chunks; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < n_chunks) { phase(wr[d], c + d, buf, d); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // ---- epilogue: the two k halves meet in LDS ([2][R][TW] fp32; the A tiles are dead), then RoPE + rounding + row writes -------------
    float *ex = reinterpret_cast<float *>(gemm_lds);
    __syncthreads();
    if (streams) {
#pragma unroll
        for (int mt = 0; mt < RT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) ex[(kh * R + 16 * mt + 4 * g + r) * TW + 16 * cg + n] = acc[mt][r];     // C layout: lane holds rows 4g + r of column n
    }
    __syncthreads();
    // v_t (round 6): the V cache is transposed ([H_kv][128][max_len], samd_tree_attention_vt); a tile of V columns then walks its (row, pair)
    // items row-fastest, so that neighbouring lanes write neighbouring keys of one V^T row
    const bool vt_tile = v_t && ((PP * (int)blockIdx.x) >> 6) >= H + Hkv;
    for (int i = tid; i < R * PP; i += NT) {
        const int row = vt_tile ? i % R : i / PP, p = vt_tile ? i / R : i % PP;
        if (row >= n_rows || L + row >= max_len) continue;                     // rows past the draft / past the cache are not written (k_rope_kv)
        // sums rounded to the model dtype first, as the projection's own output would have been (k_rope_kv does the same on partials)
        const float x1 = (float)(E)(ex[row * TW + p] + ex[(R + row) * TW + p]);
        const float x2 = (float)(E)(ex[row * TW + PP + p] + ex[(R + row) * TW + PP + p]);
        const int pair = PP * (int)blockIdx.x + p, head = pair >> 6, j = pair & 63;   // global pair index -> head, position inside it (j and j + 64)
        if (head >= H + Hkv) {                                                    // V: plain rows
            if (v_t) {
                E *dst = v_cache + (size_t)(head - H - Hkv) * max_len * 128 + L + row;
                dst[(size_t)j * max_len] = (E)x1; dst[(size_t)(j + 64) * max_len] = (E)x2;
                continue;
            }
            E *dst = v_cache + ((size_t)(head - H - Hkv) * max_len + L + row) * 128;
            dst[j] = (E)x1; dst[j + 64] = (E)x2;
            continue;
        }
        const float c = cs[(size_t)row * 128 + j], sn = cs[(size_t)row * 128 + 64 + j];
        const E o1 = (E)(x1 * c - x2 * sn), o2 = (E)(x2 * c + x1 * sn);
        E *dst = head < H ? q_out + ((size_t)row * H + head) * 128 : k_cache + ((size_t)(head - H) * max_len + L + row) * 128;
        dst[j] = o1; dst[j + 64] = o2;
    }
}

// row-major [N][K] -> the packed tile layout of k_gemm_qkv_rope<CG> (16 CG columns per tile), with the rotate_half row permutation:
// pairs are numbered head by head (pair P = 64 head + j stands for head columns j and 64 + j); tile t holds pairs [8 CG t, 8 CG (t + 1)) --
// packed row 16 CG t + q = the FIRST column of pair 8 CG t + q for q < 8 CG, the SECOND column of pair 8 CG t + q - 8 CG otherwise.
//   block (tile t, chunk c) = CG x 8 KiB contiguous at ((t * K/256 + c) * 512 CG) uint4 units; unit (2 bl + j) * 128 CG + x holds
//   Wperm[16 CG t + 16 cg + n][256 c + 64 (2 kh + bl) + 16 g + 8 j .. +7] for x = 64 (CG kh + cg) + 16 g + n.
template <int CG>
__global__ __launch_bounds__(256) void k_gemm_pack_qkv(const uint4 *__restrict__ W, uint4 *__restrict__ out, int N, int K) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)N * K / 8;
    if (u >= total) return;
    constexpr int PP = 8 * CG;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u / (512 * CG);
    const int in = (int)(u % (512 * CG)), jj = in / (128 * CG), x = in % (128 * CG), w = x >> 6, g = (x >> 4) & 3, n = x & 15, cg = w % CG, kh = w / CG;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks), bl = jj >> 1, j = jj & 1;
    const int q = 16 * cg + n, pair = PP * t + (q < PP ? q : q - PP);
    const long long row = 128LL * (pair >> 6) + (pair & 63) + (q < PP ? 0 : 64), col = 256LL * c + 64 * (2 * kh + bl) + 16 * g + 8 * j;
    out[u] = W[(row * K + col) / 8];
}

// 48-column tiles (3 column groups) when they divide the matrix and need no more rounds of workgroups over the CUs than 64-column tiles:
// Vicuna-7B's 12288 q|k|v columns = 256 tiles of 48 = one workgroup on every CU (64-column tiles: 192 workgroups, a quarter of the CUs idle
// in a launch bound by what a CU's memory pipe ingests); Vicuna-13B's 15360 = 320 x 48 (two rounds) or 240 x 64 (one): 64.
static int qkv_tile_groups(int n_heads_total) {
    static const int env = [] { const char *e = getenv("SAMD_QKV_TILE"); return e ? atoi(e) : 0; }();
    const int n_cu = samd_cu_count();
    const int N = n_heads_total * 128;
    if (N % 48 != 0 || env == 64) return 4;
    if (env == 48) return 3;
    const int t48 = N / 48, t64 = N / 64;
    return ((t48 + n_cu - 1) / n_cu) * 48 < ((t64 + n_cu - 1) / n_cu) * 64 ? 3 : 4;
}

// ================================================================================================
// gate|up projection + SiLU*up on ALL CUs (round 3).  k_gemm_skinny<EPI = 1> covers gate|up with 128-column tiles: 172 workgroups for
// Vicuna-7B's 2 x 11008 columns, and a launch on 172 CUs streams at 172 x ~36 GB/s = 6.0 TB/s -- what a CU's memory pipe ingests,
// not what HBM delivers (profiles/r03_gemm_variants.md).  Here the unit of work is a PAIR = 16 gate columns + the 16 up columns they
// multiply (two MFMA column groups, two waves): 688 pairs are dealt out evenly, 2 or 3 to each of 256 workgroups, so every CU pulls.
// Waves 2i / 2i + 1 of a workgroup own pair i's gate / up group; waves beyond the workgroup's share only help staging A.
//   PACKED LAYOUT (group-major): column group gi (16 columns), chunk c: 8 KiB contiguous at ((gi * K/256 + c) * 512) uint4 units;
//   unit (2b + j) * 64 + lane holds Wg[16 gi + n][256 c + 64 b + 16 g + 8 j .. +7] for lane = 16 g + n, where Wg = the gate|up matrix with
//   its rows interleaved in groups of 16 (group 2p = gate rows 16p.., group 2p + 1 = up rows 16p..) -- samd_gemm_pack_groups.
// Stream, A staging and waits are k_gemm_skinny's (two chunks in flight, counted vmcnt, bare barriers).
// ================================================================================================
template <typename TT, int RT, int DEPTH, bool NORM, int AR = 16>          // AR: see k_gemm_qkv_rope
__global__ __launch_bounds__(64 * GEMM_WAVES, RT >= 3 || DEPTH > 2 ? 2 : GEMM_WAVES / 2) void k_gemm_pairs_silu(const typename TT::elem *__restrict__ A, const typename TT::elem *__restrict__ W,
                                                                                                     typename TT::elem *__restrict__ out, int K, int inter, int n_chunks, int n_pairs, NormArgs na) {
    typedef typename TT::elem E;
    typedef typename TT::vec8 V8;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;
    constexpr int NB = DEPTH + 1;
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, n = l & 15, g = l >> 4;
#ifdef SAMD_GEMM_ABLATE
    const int abl = samd_abl_flag;
#else
    constexpr int abl = 0;
#endif
    // this workgroup's pairs [p0, p1): an even deal of n_pairs over the grid
    const int p0 = (int)((long long)blockIdx.x * n_pairs / gridDim.x), p1 = (int)((long long)(blockIdx.x + 1) * n_pairs / gridDim.x);
    const bool active = w < 2 * (p1 - p0);                                       // wave-uniform
    static_assert(AR == 16 || (AR >= 1 && AR < 16 && NORM && RT == 1), "fewer than 16 activation rows: the norm-fold kernels only");
    const bool stager = AR == 16 || w < (AR + 1) / 2;                            // wave-uniform: a wave with a staging lane (rows 0..AR-1 belong to threads 0..32 AR - 1)
    const bool stages = !(AR & 1) ? stager : tid < 32 * AR;                      // per lane: not the upper half of an odd AR's last staging wave
    const unsigned long long stage_mask = (AR & 1) && w == AR / 2 ? 0xffffffffull : ~0ull;
    const int gi = 2 * p0 + w;                                                    // this wave's column group
    const char *wgrp = reinterpret_cast<const char *>(W) + (size_t)(active ? gi : 0) * n_chunks * 8192;
    const uint32_t wlane = (uint32_t)l * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    u32x4 wr[DEPTH][4][2];
    auto load_w = [&](u32x4 (&dst)[4][2], int c) {
        const char *p = wgrp + (size_t)c * 8192;
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int j = 0; j < 2; j++)
                asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst[b][j]) : "v"(wlane), "s"(p + 1024 * (2 * b + j)) : "memory");
    };
    // NORM: the A chunk and the norm weights of its k range come through registers and are scaled on their way to LDS (see NormArgs)
    static_assert(!NORM || RT == 1, "the norm-fold path is built for the 16-row tile");
    constexpr int XL = NORM ? 2 * XV : XV;         // memory operations per thread to stage one A chunk
    u32x4 xr[NORM ? DEPTH : 1][NORM ? XV : 1], gr[NORM ? DEPTH : 1][NORM ? XV : 1];
    __shared__ float norm_part[NORM ? (NT / 16) * 16 : 1], norm_rs[NORM ? 16 : 1];
    auto stage_x = [&](int c, int buf, int d) {
        if (!stager || (abl & 4)) return;
#pragma unroll
        for (int i = 0; i < XV; i++) {
            const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
            const E *src = A + (size_t)((abl & 8) ? (row & 15) : row) * K + (size_t)c * GEMM_KC + 8 * unit;
            if constexpr (NORM) {
                const E *gsrc = reinterpret_cast<const E *>(na.g) + (size_t)c * GEMM_KC + 8 * unit;
                if constexpr (AR & 1) norm_load_masked(xr[d][i], gr[d][i], src, gsrc, stage_mask);
                else {
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xr[d][i]) : "v"(src) : "memory");
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gr[d][i]) : "v"(gsrc) : "memory");
                }
            } else {
                E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
                asm volatile("" ::: "memory");
            }
        }
    };
    // a wave without a column group issues no weight loads, one that stages no rows no A loads: its counted waits leave those out
    auto landed = [&](int younger, int buf, int d) {
        const bool stg = stager && !(abl & 4);
        if (active) { if (stg) gemm_wait_younger<DEPTH, 8 + XL>(younger); else gemm_wait_younger<DEPTH, 8>(younger); }
        else { if (stg) gemm_wait_younger<DEPTH, XL>(younger); else gemm_wait_younger<DEPTH, 0>(younger); }
        if constexpr (NORM) {
            if (stager) {
#pragma unroll
                for (int i = 0; i < XV; i++) {
                    const int slot = tid + NT * i, row = slot >> 5;
                    // (re-defined here, behind the counted wait: the compiler does not know that the asm loads that produced them were asynchronous)
                    asm volatile("" : "+v"(xr[d][i]), "+v"(gr[d][i]) : : "memory");
                    const u32x4 v = norm_scale8<E>(xr[d][i], gr[d][i], norm_rs[row]);
                    if (stages) *reinterpret_cast<u32x4 *>(&xs[buf][0][0] + (size_t)slot * 8) = v;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (!(abl & 1)) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto phase = [&](u32x4 (&cur)[4][2], int c, int buf, int d) {
        landed(n_chunks - 1 - c, buf, d);
        if (active && !(abl & 2)) {
            const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
                u32x4 r[RT][2];
                if constexpr (RT == 1)
                    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]) : "v"(a0), "v"(a1));
                else if constexpr (RT == 2)
                    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %4 offset:8192\n\tds_read_b128 %3, %5 offset:8192\n\t"
                                 "s_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]) : "v"(a0), "v"(a1));
                else if constexpr (RT == 3)
                    asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %6 offset:8192\n\tds_read_b128 %3, %7 offset:8192\n\t"
                                 "ds_read_b128 %4, %6 offset:16384\n\tds_read_b128 %5, %7 offset:16384\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]) : "v"(a0), "v"(a1));
                else
                    asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %8 offset:8192\n\tds_read_b128 %3, %9 offset:8192\n\t"
                                 "ds_read_b128 %4, %8 offset:16384\n\tds_read_b128 %5, %9 offset:16384\n\tds_read_b128 %6, %8 offset:24576\n\t"
                                 "ds_read_b128 %7, %9 offset:24576\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]), "=&v"(r[3][0]), "=&v"(r[3][1])
                                 : "v"(a0), "v"(a1));
#pragma unroll
                for (int mt = 0; mt < RT; mt++) {
                    acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][0]), __builtin_bit_cast(V8, cur[b][0]), acc[mt]);
                    acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][1]), __builtin_bit_cast(V8, cur[b][1]), acc[mt]);
                }
            }
        }
        if (c + DEPTH < n_chunks) { if (active) load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, d); }
    };
    float norm_sv[NORM ? NORM_NS : 1];
    if constexpr (NORM) norm_issue<NT>(na, norm_sv);
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if (d < n_chunks) { if (active) load_w(wr[d], d); stage_x(d, d, d); }
    if constexpr (AR < 16) {                        // rows AR..15 of every A buffer: zero, once
        if (!stages) {
#pragma unroll
            for (int bz = 0; bz < NB; bz++) *reinterpret_cast<u32x4 *>(&xs[bz][0][0] + (size_t)tid * 8) = (u32x4){0u, 0u, 0u, 0u};
        }
    }
    if constexpr (NORM) {                           // the partial sums were requested before the chunks (see k_gemm_qkv_rope)
        if (n_chunks >= DEPTH) {
            if (active) { if (stager) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * (8 + XL)) : "memory"); else asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * 8) : "memory"); }
            else { if (stager) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH * XL) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); }
        } else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        norm_finish<NT>(na, norm_sv, norm_part, norm_rs);
    }
    {
        int buf = 0;
        for (int c = 0; c < n_chunks; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < n_chunks) { phase(wr[d], c + d, buf, d); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // ---- epilogue: the up waves hand their values over through LDS, the gate waves write silu(gate) * up ---------------------------------
    float *ex = reinterpret_cast<float *>(gemm_lds);                            // [4 pairs][R][16]; the A tiles are dead
    __syncthreads();
    if (active && (w & 1)) {
#pragma unroll
        for (int mt = 0; mt < RT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) ex[((w >> 1) * R + 16 * mt + 4 * g + r) * 16 + n] = acc[mt][r];
    }
    __syncthreads();
    if (active && !(w & 1)) {
        const int col = 16 * (p0 + (w >> 1)) + n;
#pragma unroll
        for (int mt = 0; mt < RT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = 16 * mt + 4 * g + r;
                // the roundings of HF's act_fn(gate_proj(x)) * up_proj(x) in the model dtype (same as k_silu_mul)
                const float gf = (float)(E)acc[mt][r], uf = (float)(E)ex[((w >> 1) * R + m) * 16 + n];
                const E sv = (E)(gf / (1.f + __expf(-gf)));
                out[(size_t)m * inter + col] = (E)((float)sv * uf);
            }
    }
}

// ================================================================================================
// Complete-sum projection with the residual add as its epilogue (round 3, the "norm-fold" forward): x[m][n] <- x[m][n] + (A W^T)[m][n] for
// o_proj / down_proj at 16 rows, plus the row's sum of squares over the workgroup's 16 columns -- what the CONSUMING projection needs to
// apply the RMSNorm itself (k_gemm_qkv_rope / k_gemm_pairs_silu with NORM), so that the two k_rmsnorm launches of a decoder layer and the
// fp32 split-K partials they read disappear.  One workgroup per 16 output columns and ALL of K: wave w takes the 256-k chunks w, w + 8, ...
// with its own LDS-DMA'd A chunks (no barrier in the stream), the eight partial accumulators meet in LDS in a fixed order.
//   W: group-major packed (samd_gemm_pack_groups of the plain [N][K] matrix); ssq: [N / 16][16] fp32 (tile-major, row m at [t][m]).
// Roundings are the reference's: the projection's output in the model dtype, then the residual sum in the model dtype
// (LlamaDecoderLayer: hidden_states = residual + hidden_states), squares of the stored values (LlamaRMSNorm: x.float().pow(2)).
// ================================================================================================
// EARLY (seam experiment, scripts/seam_probe.py / profiles/r04_attention.md section 5; K = 4096 only: two chunks per wave): the launch runs
// on a second queue BESIDE the attention launches that produce A.  Every wave requests ALL of its weights at entry, then the workgroup
// polls `counter` -- the producers' arrival count -- until this workgroup's own epoch says A is complete, and only then requests A.
template <typename TT, int ROWS, bool EARLY = false>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_gemm_cs_residual(const typename TT::elem *__restrict__ A, const typename TT::elem *__restrict__ W,
                                                                           typename TT::elem *__restrict__ x, float *__restrict__ ssq, int K, int N, int n_chunks,
                                                                           const int *__restrict__ counter = nullptr, int *__restrict__ epoch = nullptr,
                                                                           int arrivals = 0) {
    typedef typename TT::elem E;
    typedef typename TT::vec8 V8;
    constexpr int CSD = 2;                                     // chunks in flight per wave
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, n = l & 15, g = l >> 4;
    E *xs = reinterpret_cast<E *>(gemm_lds) + (size_t)w * CSD * 16 * GEMM_KC;          // this wave's CSD buffers of [16][256]
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)xs;
    const char *wgrp = reinterpret_cast<const char *>(W) + (size_t)blockIdx.x * n_chunks * 8192;
    const uint32_t wlane = (uint32_t)l * 16;

    // ROWS < 16: a draft of ROWS rows -- only rows 0..ROWS-1 of the activation tile are fetched (at 8 rows half of what this ingest-bound
    // launch pulls from L2 besides its weights); rows ROWS..15 of the LDS tiles are zeroed once and their outputs are not written.  A load
    // covers two rows (lanes 0-31 | 32-63): with an odd ROWS the upper half of the last one is masked off -- the wave still issues the
    // instruction, so the counted waits below do not change
    static_assert(ROWS >= 1 && ROWS <= 16, "");
    constexpr int AL = (ROWS + 1) / 2;                         // A loads per lane and chunk
    if constexpr (ROWS < 16) {
#pragma unroll
        for (int buf = 0; buf < CSD; buf++)
#pragma unroll
            for (int i = ROWS / 2; i < 8; i++)
                if (!(ROWS & 1) || i > ROWS / 2 || l >= 32)
                    *reinterpret_cast<u32x4 *>(xs + (size_t)buf * 16 * GEMM_KC + (size_t)(64 * i + l) * 8) = (u32x4){0u, 0u, 0u, 0u};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    floatx4 acc = (floatx4){0.f, 0.f, 0.f, 0.f};
    u32x4 wr[CSD][4][2];
    auto issue_w = [&](u32x4 (&dst)[4][2], int c) {
        const char *p = wgrp + (size_t)c * 8192;
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int j = 0; j < 2; j++)
                asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst[b][j]) : "v"(wlane), "s"(p + 1024 * (2 * b + j)) : "memory");
    };
    auto issue_a = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < AL; i++) {                         // the wave's own A chunk: 32 units of 16 B per row, unit u of row r at position u ^ (r & 15)
            const int slot = l + 64 * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
            const E *src = A + (size_t)row * K + (size_t)c * GEMM_KC + 8 * unit;
            E *dst_l = xs + (size_t)buf * 16 * GEMM_KC + (size_t)(64 * i) * 8;
            if ((ROWS & 1) && i == AL - 1) { if (l < 32) __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst_l, 16, 0, 0); }   // (row ROWS is not fetched)
            else __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst_l, 16, 0, 0);
            asm volatile("" ::: "memory");
        }
    };
    auto issue = [&](u32x4 (&dst)[4][2], int c, int buf) { issue_w(dst, c); issue_a(c, buf); };
    auto phase = [&](u32x4 (&cur)[4][2], int c, int buf, bool more) {
        // EARLY: both chunks' weights are older than any A load, so what may still fly while chunk 0 is consumed is chunk 1's A only
        if (more) { if constexpr (EARLY) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(AL) : "memory"); else asm volatile("s_waitcnt vmcnt(%0)" : : "n"(8 + AL) : "memory"); }
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (16 * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r0, r1;
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r0), "=&v"(r1) : "v"(a0), "v"(a1));
            acc = TT::mfma(__builtin_bit_cast(V8, r0), __builtin_bit_cast(V8, cur[b][0]), acc);
            acc = TT::mfma(__builtin_bit_cast(V8, r1), __builtin_bit_cast(V8, cur[b][1]), acc);
        }
    };
    // chunks of this wave: w, w + 8, ...; two in flight, the LDS buffer of a chunk is refilled only after its reads (lgkmcnt(0) above)
    const int mine = (n_chunks - w + GEMM_WAVES - 1) / GEMM_WAVES;
    if constexpr (EARLY) {
        if (mine > 0) issue_w(wr[0], w);
        if (mine > 1) issue_w(wr[1], w + GEMM_WAVES);
        __shared__ int my_epoch;
        if (tid == 0) {
            const int e = epoch[blockIdx.x];
            const int target = (e + 1) * arrivals;
            for (int spin = 0; spin < (1 << 22); spin++) {                 // bounded: a lost producer ends in wrong sums, not in a hung GPU
                if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) break;
                __builtin_amdgcn_s_sleep(4);
            }
            my_epoch = e;
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (mine > 0) issue_a(w, 0);
        if (mine > 1) issue_a(w + GEMM_WAVES, 1);
        if (mine > 0) phase(wr[0], w, 0, mine > 1);
        if (mine > 1) phase(wr[1], w + GEMM_WAVES, 1, false);
        if (tid == 0) epoch[blockIdx.x] = my_epoch + 1;
    } else {
        if (mine > 0) issue(wr[0], w, 0);
        if (mine > 1) issue(wr[1], w + GEMM_WAVES, 1);
        for (int i = 0; i < mine; i += 2) {
            phase(wr[0], w + GEMM_WAVES * i, 0, i + 1 < mine);
            if (i + 2 < mine) issue(wr[0], w + GEMM_WAVES * (i + 2), 0);
            if (i + 1 < mine) {
                phase(wr[1], w + GEMM_WAVES * (i + 1), 1, i + 2 < mine);
                if (i + 3 < mine) issue(wr[1], w + GEMM_WAVES * (i + 3), 1);
            }
        }
    }
    // ---- the eight k shares meet in LDS (the A buffers are dead), summed in wave order; residual, rounding, row sums of squares -----------
    __syncthreads();
    float *ex = reinterpret_cast<float *>(gemm_lds);                               // [8][16][16]
#pragma unroll
    for (int r = 0; r < 4; r++) ex[(w * 16 + 4 * g + r) * 16 + n] = acc[r];        // C layout: lane holds rows 4g + r of column n
    __syncthreads();
    if (tid < 16 * ROWS) {
        const int row = tid >> 4, col = tid & 15;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < GEMM_WAVES; k++) sum += ex[(k * 16 + row) * 16 + col];
        E *xp = x + (size_t)row * N + 16 * blockIdx.x + col;
        const E o = (E)sum;
        const E y = (E)((float)*xp + (float)o);
        *xp = y;
        float q = (float)y * (float)y;
        q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4); q += __shfl_xor(q, 8);
        if (col == 0) ssq[(size_t)blockIdx.x * 16 + row] = q;
    }
}

// row-major [N][K] -> group-major packed layout of k_gemm_pairs_silu (rows already in group order); one thread moves one 16-byte unit
__global__ __launch_bounds__(256) void k_gemm_pack_groups(const uint4 *__restrict__ W, uint4 *__restrict__ out, int N, int K) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)N * K / 8;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 9;                                    // 512 units per 8 KiB block
    const int in = (int)(u & 511), jj = in >> 6, lane = in & 63, g = lane >> 4, n = lane & 15, b = jj >> 1, j = jj & 1;
    const long long gi = blk / n_chunks; const int c = (int)(blk % n_chunks);
    const long long row = 16 * gi + n, col = 256LL * c + 64 * b + 16 * g + 8 * j;
    out[u] = W[(row * K + col) / 8];
}

// row-major [N][K] (2-byte elements) -> packed blocks; one thread moves one 16-byte unit
__global__ __launch_bounds__(256) void k_gemm_pack(const uint4 *__restrict__ W, uint4 *__restrict__ out, int N, int K) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;          // destination unit
    const long long total = (long long)N * K / 8;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 12;
    const int in = (int)(u & 4095), jj = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks), b = jj >> 1, j = jj & 1;
    const long long row = 128LL * t + 16 * w + n, col = 256LL * c + 64 * b + 16 * g + 8 * j;
    out[u] = W[(row * K + col) / 8];
}

// DEPTH = 2 chunks in flight at every row tile.  Three (128 KiB of LDS at 64 rows) measured SLOWER: gate|up 40.3 vs 38.8 us at 64
// rows, 34.9 vs 34.5 at 32 -- the launch is not short of requests in flight (profiles/r02_gemm_rows64.md).
template <typename TT, int RT, int EPI, int DEPTH, bool GM = false>
static hipError_t gemm_launch(dim3 grid, hipStream_t st, const void *A, const void *W, float *partial, void *out, int K, int N, int chunks, int splits) {
    constexpr int lds = (DEPTH + 1) * 16 * RT * GEMM_KC * 2;
    if constexpr (lds > 65536) {
        static unsigned long long done = 0ull;                     // per-device (samd_common.h)
        const hipError_t attr = samd_reserve_lds((const void *)k_gemm_skinny<TT, RT, EPI, DEPTH, GM>, lds, &done);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL((k_gemm_skinny<TT, RT, EPI, DEPTH, GM>), grid, dim3(64 * GEMM_WAVES), lds, st, (const typename TT::elem *)A, (const typename TT::elem *)W, partial,
                       (typename TT::elem *)out, K, N, chunks, splits);
    return hipSuccess;
}

template <int EPI, bool GM = false>
static hipError_t gemm_dispatch(int dtype, int rows_pad, dim3 grid, hipStream_t st, const void *A, const void *W, float *partial, void *out, int K, int N, int chunks,
                                int splits) {
#define GO(TT, RT, D) return gemm_launch<TT, RT, EPI, D, GM>(grid, st, A, W, partial, out, K, N, chunks, splits)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1, 2); else if (rows_pad == 32) GO(TT, 2, 2); else if (rows_pad == 48) GO(TT, 3, 2); else GO(TT, 4, 2); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
}

template <typename TT, int RT, int DEPTH, int CG, bool NORM = false, int AR = 16>
static hipError_t qkv_rope_launch(hipStream_t st, const void *A, const void *W, int K, int tiles, const float *cs, const int *d_L, const int *d_n, void *q, void *k, void *v,
                                  int H, int Hkv, long long max_len, int v_t, NormArgs na = NormArgs{nullptr, nullptr, 0, 0.f, 0.f}) {
    constexpr int lds_a = (DEPTH + 1) * 16 * RT * GEMM_KC * 2, lds_e = 2 * 16 * RT * 16 * CG * 4, lds = lds_a > lds_e ? lds_a : lds_e;
    if constexpr (lds > 60000) {
        static unsigned long long done = 0ull;
        const hipError_t attr = samd_reserve_lds((const void *)k_gemm_qkv_rope<TT, RT, DEPTH, CG, NORM, AR>, lds + 4096, &done);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL((k_gemm_qkv_rope<TT, RT, DEPTH, CG, NORM, AR>), dim3(tiles), dim3(64 * GEMM_WAVES), lds, st, (const typename TT::elem *)A, (const typename TT::elem *)W, K, K / GEMM_KC,
                       cs, d_L, d_n, (typename TT::elem *)q, (typename TT::elem *)k, (typename TT::elem *)v, H, Hkv, max_len, na, v_t);
    return hipSuccess;
}

template <typename TT, int RT, int DEPTH, bool NORM = false, int AR = 16>
static hipError_t pairs_silu_launch(hipStream_t st, int grid, const void *A, const void *W, void *out, int K, int inter, int n_pairs,
                                    NormArgs na = NormArgs{nullptr, nullptr, 0, 0.f, 0.f}) {
    constexpr int lds_a = (DEPTH + 1) * 16 * RT * GEMM_KC * 2, lds_e = 4 * 16 * RT * 16 * 4, lds = lds_a > lds_e ? lds_a : lds_e;
    if constexpr (lds > 60000) {
        static unsigned long long done = 0ull;
        const hipError_t attr = samd_reserve_lds((const void *)k_gemm_pairs_silu<TT, RT, DEPTH, NORM, AR>, lds + 4096, &done);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL((k_gemm_pairs_silu<TT, RT, DEPTH, NORM, AR>), dim3(grid), dim3(64 * GEMM_WAVES), lds, st, (const typename TT::elem *)A, (const typename TT::elem *)W,
                       (typename TT::elem *)out, K, inter, K / GEMM_KC, n_pairs, na);
    return hipSuccess;
}

// activation rows the norm-fold projections can fetch: the two tile forms (8, 16) and the headline workload's two commonest draft
// sizes (5 and 9 nodes: 75 % and 16 % of its steps, profiles/rows_exact.md)
static bool samd_rows_fetch_ok(int rows) { return rows == 5 || rows == 8 || rows == 9 || rows == 16; }

extern "C" {

// choose the split-K factor.  Measured (scripts/gemm_bench.py, profiles/): the stream is fastest when the launch is ONE
// balanced wave of workgroups -- at most one per CU, each with a long run of chunks (gate|up: 172 workgroups x 16 chunks
// 5.47 TB/s, lm_head 250 x 16 5.92 TB/s; QKV 96 x 2 splits 5.15 TB/s vs 4.9 with 4 or 8) -- so: the largest split count
// that keeps columns x splits <= 256 and leaves every split at least one chunk.  Fewer splits also mean fewer fp32
// partials for the consumer to add up; capped at 8 (whole forward at 64 rows: 4.47 ms with cap 8, 4.56 with 6, 4.64 with 4).
// The two tuning knobs (SAMD_GEMM_SPLIT_CAP, SAMD_GEMM_SPLITS) are read ONCE, at the first call: callers size their fp32
// partial-sum workspaces from this function's answer, so the answer for a shape must not change during the process.
int samd_gemm_splits(int32_t N, int32_t K, int32_t rows_pad) {
    static const int env_cap = [] { const char *e = getenv("SAMD_GEMM_SPLIT_CAP"); const int v = e ? atoi(e) : 8; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
    static const int env_fixed = [] { const char *e = getenv("SAMD_GEMM_SPLITS"); const int v = e ? atoi(e) : 0; return v < 0 ? 0 : (v > 8 ? 8 : v); }();
    const int cols = N / GEMM_COLS, chunks = K / GEMM_KC;
    (void)rows_pad;
    if (env_fixed) return env_fixed > chunks ? (chunks < 1 ? 1 : chunks) : env_fixed;
    int s = 256 / (cols > 0 ? cols : 1);
    if (s > env_cap) s = env_cap;
    if (s > chunks) s = chunks;
    return s < 1 ? 1 : s;
}

int64_t samd_gemm_workspace(int32_t rows_pad, int32_t N, int32_t splits) { return (int64_t)splits * rows_pad * N * 4; }

// out (dtype, [rows_pad][N]) when splits == 1, else fp32 partials [splits][rows_pad][N] in d_partial.
// rows_pad in {16, 32, 48, 64}; A must hold rows_pad rows (pad rows are read, their products land in pad rows).
int samd_gemm_skinny_silu(const void *d_A, const void *d_W, int32_t rows_pad, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_W || !d_out || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_skinny_silu: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0) or null pointer"); return SAMD_E_INVALID;
    }
    const hipError_t e = gemm_dispatch<1>(dtype, rows_pad, dim3(N / GEMM_COLS, 1), (hipStream_t)stream, d_A, d_W, nullptr, d_out, K, N, K / GEMM_KC, 1);
    if (e != hipSuccess) { samd_set_error("samd_gemm_skinny_silu: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pack_weights(const void *d_W, void *d_packed, int32_t N, int32_t K, void *stream) {
    if (!d_W || !d_packed || d_W == d_packed || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_gemm_pack_weights: needs N %% 128 == 0, K %% 256 == 0 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 8;
    hipLaunchKernelGGL(k_gemm_pack, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W, (uint4 *)d_packed, N, K);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pack_groups(const void *d_W, void *d_packed, int32_t N, int32_t K, void *stream) {
    if (!d_W || !d_packed || d_W == d_packed || N < 16 || N % 16 != 0 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_gemm_pack_groups: needs N %% 16 == 0, K %% 256 == 0 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 8;
    hipLaunchKernelGGL(k_gemm_pack_groups, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W, (uint4 *)d_packed, N, K);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pairs_silu_norm(const void *d_x, const float *d_ssq, const void *d_norm_weight, float eps, const void *d_Wg, int32_t rows_pad, int32_t inter, int32_t K,
                              void *d_out, int32_t dtype, void *stream) {
    if (!d_x || !d_ssq || !d_norm_weight || !d_Wg || !d_out || !samd_rows_fetch_ok(rows_pad) || inter < 16 || inter % 16 != 0 || K < GEMM_KC || K % GEMM_KC != 0 ||
        K / 16 > 32 * NORM_NS || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_pairs_silu_norm: unsupported shape (5, 8, 9 or 16 rows, inter %% 16 == 0, K %% 256 == 0, K <= 8192, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    const int n_cu = samd_cu_count();
    const int n_pairs = inter / 16;
    int grid = n_pairs < n_cu ? n_pairs : n_cu;
    while ((n_pairs + grid - 1) / grid > 4) grid += n_cu;
    const NormArgs na{d_ssq, d_norm_weight, K / 16, 1.f / (float)K, eps};
    hipStream_t st = (hipStream_t)stream;
    // rows_pad < 16: a draft of that many nodes -- only rows 0..rows_pad-1 of x are fetched (the tile stays 16 rows; outputs of the others are zero)
    hipError_t e = hipSuccess;
#define GO(TT, AR) e = pairs_silu_launch<TT, 1, 3, true, AR>(st, grid, d_x, d_Wg, d_out, K, inter, n_pairs, na)
#define ROWS(TT) do { if (rows_pad == 5) GO(TT, 5); else if (rows_pad == 8) GO(TT, 8); else if (rows_pad == 9) GO(TT, 9); else GO(TT, 16); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_pairs_silu_norm: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_cs_residual(const void *d_A, const void *d_Wg, int32_t rows_pad, int32_t N, int32_t K, void *d_x, float *d_ssq, int32_t dtype, void *stream) {
    if (!d_A || !d_Wg || !d_x || !d_ssq || !samd_rows_fetch_ok(rows_pad) || N < 16 || N % 16 != 0 || K < GEMM_KC || K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_cs_residual: unsupported shape (5, 8, 9 or 16 rows, N %% 16 == 0, K %% 256 == 0, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    constexpr int lds = GEMM_WAVES * 2 * 16 * GEMM_KC * 2;                       // 128 KiB: two A chunks per wave
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
#define GO(TT, ROWS, ET) do { static unsigned long long done = 0ull; \
        e = samd_reserve_lds((const void *)k_gemm_cs_residual<TT, ROWS>, lds, &done); \
        if (e == hipSuccess) hipLaunchKernelGGL((k_gemm_cs_residual<TT, ROWS>), dim3(N / 16), dim3(64 * GEMM_WAVES), lds, st, (const ET *)d_A, (const ET *)d_Wg, (ET *)d_x, d_ssq, K, N, K / GEMM_KC, (const int *)nullptr, (int *)nullptr, 0); } while (0)
#define ROWS(TT, ET) do { if (rows_pad == 5) GO(TT, 5, ET); else if (rows_pad == 8) GO(TT, 8, ET); else if (rows_pad == 9) GO(TT, 9, ET); else GO(TT, 16, ET); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16, _Float16); else ROWS(GBF16, __bf16);
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_cs_residual: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

/* seam experiment hook (scripts/seam_probe.py): samd_gemm_cs_residual for o_proj (K = 4096, <= 8 rows) launched on a SECOND stream beside the
 * attention launches; it requests its weights at entry and polls d_counter (samd_tree_attention_signal's arrivals) before it touches A.
 * d_epoch int32[N / 16], zero-initialised, owned by the caller; arrivals = n_q_pad * n_heads of the producing merge launch. */
int samd_gemm_cs_residual_early(const void *d_A, const void *d_Wg, int32_t N, int32_t K, void *d_x, float *d_ssq, int32_t dtype, const int32_t *d_counter,
                                int32_t *d_epoch, int32_t arrivals, void *stream) {
    if (!d_A || !d_Wg || !d_x || !d_ssq || !d_counter || !d_epoch || arrivals < 1 || N < 16 || N % 16 != 0 || K != 2 * GEMM_WAVES * GEMM_KC ||
        (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_cs_residual_early: unsupported shape (K must be 4096, N %% 16 == 0, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    constexpr int lds = GEMM_WAVES * 2 * 16 * GEMM_KC * 2;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (dtype == SAMD_F16) {
        static unsigned long long done = 0ull;
        e = samd_reserve_lds((const void *)k_gemm_cs_residual<GF16, 8, true>, lds, &done);
        if (e == hipSuccess) hipLaunchKernelGGL((k_gemm_cs_residual<GF16, 8, true>), dim3(N / 16), dim3(64 * GEMM_WAVES), lds, st, (const _Float16 *)d_A, (const _Float16 *)d_Wg,
                                                (_Float16 *)d_x, d_ssq, K, N, K / GEMM_KC, d_counter, d_epoch, arrivals);
    } else {
        static unsigned long long done = 0ull;
        e = samd_reserve_lds((const void *)k_gemm_cs_residual<GBF16, 8, true>, lds, &done);
        if (e == hipSuccess) hipLaunchKernelGGL((k_gemm_cs_residual<GBF16, 8, true>), dim3(N / 16), dim3(64 * GEMM_WAVES), lds, st, (const __bf16 *)d_A, (const __bf16 *)d_Wg,
                                                (__bf16 *)d_x, d_ssq, K, N, K / GEMM_KC, d_counter, d_epoch, arrivals);
    }
    if (e != hipSuccess) { samd_set_error("samd_gemm_cs_residual_early: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pairs_silu(const void *d_A, const void *d_Wg, int32_t rows_pad, int32_t inter, int32_t K, void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_Wg || !d_out || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || inter < 16 || inter % 16 != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_pairs_silu: unsupported shape (rows 16/32/48/64, inter %% 16 == 0, K %% 256 == 0, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    // one workgroup per CU (256 on MI355X) with an even share of the pairs; more workgroups only when a share would exceed 4 pairs (8 waves)
    const int n_cu = samd_cu_count();
    const int n_pairs = inter / 16;
    int grid = n_pairs < n_cu ? n_pairs : n_cu;
    while ((n_pairs + grid - 1) / grid > 4) grid += n_cu;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    static const int depth_env = [] { const char *e = getenv("SAMD_PAIRS_DEPTH"); return e ? atoi(e) : 0; }();
#ifdef SAMD_GEMM_ABLATE
    static const int abl_set = [] { const char *e = getenv("SAMD_GEMM_ABL"); const int v = e ? atoi(e) : 0; return hipMemcpyToSymbol(HIP_SYMBOL(samd_abl_flag), &v, 4) == hipSuccess ? 1 : -1; }();
    (void)abl_set;
#endif
#define ARGS st, grid, d_A, d_Wg, d_out, K, inter, n_pairs
#define GO(TT) (rows_pad == 16 ? (depth_env == 2 ? pairs_silu_launch<TT, 1, 2>(ARGS) : depth_env == 4 ? pairs_silu_launch<TT, 1, 4>(ARGS) : pairs_silu_launch<TT, 1, 3>(ARGS)) \
                : rows_pad == 32 ? (depth_env == 2 ? pairs_silu_launch<TT, 2, 2>(ARGS) : pairs_silu_launch<TT, 2, 3>(ARGS)) \
                : rows_pad == 48 ? pairs_silu_launch<TT, 3, 2>(ARGS) : pairs_silu_launch<TT, 4, 2>(ARGS))
    e = dtype == SAMD_F16 ? GO(GF16) : GO(GBF16);
#undef GO
#undef ARGS
    if (e != hipSuccess) { samd_set_error("samd_gemm_pairs_silu: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pack_qkv64(const void *d_W, void *d_packed, int32_t n_heads_total, int32_t K, void *stream) {
    if (!d_W || !d_packed || d_W == d_packed || n_heads_total < 1 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_gemm_pack_qkv64: needs K %% 256 == 0, whole 128-column heads and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)n_heads_total * 128 * K / 8;
    if (qkv_tile_groups(n_heads_total) == 3)
        hipLaunchKernelGGL(k_gemm_pack_qkv<3>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W, (uint4 *)d_packed, n_heads_total * 128, K);
    else
        hipLaunchKernelGGL(k_gemm_pack_qkv<4>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W, (uint4 *)d_packed, n_heads_total * 128, K);
    LAUNCHCHK();
    return SAMD_OK;
}

static int gemm_qkv_rope_impl(const void *d_A, const void *d_W64, int32_t rows_pad, int32_t K, const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n,
                              void *d_q_out, void *d_k_cache, void *d_v_cache, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len,
                              int32_t dtype, void *stream, int v_t) {
    if (!d_A || !d_W64 || !d_cs || !d_cache_length || !d_n || !d_q_out || !d_k_cache || !d_v_cache || head_dim != 128 || n_heads < 1 || n_kv_heads < 1 ||
        (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || K < GEMM_KC || K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_qkv_rope: unsupported shape (rows 16/32/48/64, head_dim 128, K %% 256 == 0, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    static const int depth_env = [] { const char *e = getenv("SAMD_QKV_DEPTH"); return e ? atoi(e) : 0; }();
    const int groups = qkv_tile_groups(n_heads + 2 * n_kv_heads);
    const int tiles = (n_heads + 2 * n_kv_heads) * 128 / (16 * groups);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
#define GO(TT, RT, D, CG) e = qkv_rope_launch<TT, RT, D, CG>(st, d_A, d_W64, K, tiles, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_v_cache, n_heads, n_kv_heads, (long long)max_len, v_t)
#define ROWS(TT, CG) do { if (rows_pad == 16) { if (depth_env == 2) GO(TT, 1, 2, CG); else if (depth_env == 3) GO(TT, 1, 3, CG); else GO(TT, 1, 4, CG); } \
                          else if (rows_pad == 32) { if (depth_env == 2) GO(TT, 2, 2, CG); else GO(TT, 2, 4, CG); } \
                          else if (rows_pad == 48) GO(TT, 3, 3, CG); else GO(TT, 4, 3, CG); } while (0)
    if (groups == 3) { if (dtype == SAMD_F16) ROWS(GF16, 3); else ROWS(GBF16, 3); }
    else { if (dtype == SAMD_F16) ROWS(GF16, 4); else ROWS(GBF16, 4); }
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_qkv_rope: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_qkv_rope(const void *d_A, const void *d_W64, int32_t rows_pad, int32_t K, const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n,
                       void *d_q_out, void *d_k_cache, void *d_v_cache, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len,
                       int32_t dtype, void *stream) {
    return gemm_qkv_rope_impl(d_A, d_W64, rows_pad, K, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_v_cache, n_heads, n_kv_heads, head_dim, max_len, dtype, stream, 0);
}

/* round 6: the same with the V rows written into a TRANSPOSED cache, d_vt_cache [H_kv][128][max_len] (what samd_tree_attention_vt reads) */
int samd_gemm_qkv_rope_vt(const void *d_A, const void *d_W64, int32_t rows_pad, int32_t K, const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n,
                          void *d_q_out, void *d_k_cache, void *d_vt_cache, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len,
                          int32_t dtype, void *stream) {
    return gemm_qkv_rope_impl(d_A, d_W64, rows_pad, K, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_vt_cache, n_heads, n_kv_heads, head_dim, max_len, dtype, stream, 1);
}

static int gemm_qkv_rope_norm_impl(const void *d_x, const float *d_ssq, const void *d_norm_weight, float eps, const void *d_W64, int32_t rows_pad, int32_t K,
                                   const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n, void *d_q_out, void *d_k_cache, void *d_v_cache,
                                   int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len, int32_t dtype, void *stream, int v_t) {
    if (!d_x || !d_ssq || !d_norm_weight || !d_W64 || !d_cs || !d_cache_length || !d_n || !d_q_out || !d_k_cache || !d_v_cache || head_dim != 128 || n_heads < 1 ||
        n_kv_heads < 1 || !samd_rows_fetch_ok(rows_pad) || K < GEMM_KC || K % GEMM_KC != 0 || K / 16 > 32 * NORM_NS || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_qkv_rope_norm: unsupported shape (5, 8, 9 or 16 rows, head_dim 128, K %% 256 == 0, K <= 8192, f16/bf16) or null pointer"); return SAMD_E_INVALID;
    }
    const int groups = qkv_tile_groups(n_heads + 2 * n_kv_heads);
    const int tiles = (n_heads + 2 * n_kv_heads) * 128 / (16 * groups);
    const NormArgs na{d_ssq, d_norm_weight, K / 16, 1.f / (float)K, eps};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
#define GO(TT, CG, AR) e = qkv_rope_launch<TT, 1, 4, CG, true, AR>(st, d_x, d_W64, K, tiles, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_v_cache, n_heads, n_kv_heads, (long long)max_len, v_t, na)
    // rows_pad < 16: a draft of that many nodes -- only rows 0..rows_pad-1 of x are fetched (the tile stays 16 rows)
#define ROWS(TT, CG) do { if (rows_pad == 5) GO(TT, CG, 5); else if (rows_pad == 8) GO(TT, CG, 8); else if (rows_pad == 9) GO(TT, CG, 9); else GO(TT, CG, 16); } while (0)
    if (groups == 3) { if (dtype == SAMD_F16) ROWS(GF16, 3); else ROWS(GBF16, 3); }
    else { if (dtype == SAMD_F16) ROWS(GF16, 4); else ROWS(GBF16, 4); }
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_qkv_rope_norm: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_qkv_rope_norm(const void *d_x, const float *d_ssq, const void *d_norm_weight, float eps, const void *d_W64, int32_t rows_pad, int32_t K,
                            const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n, void *d_q_out, void *d_k_cache, void *d_v_cache,
                            int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len, int32_t dtype, void *stream) {
    return gemm_qkv_rope_norm_impl(d_x, d_ssq, d_norm_weight, eps, d_W64, rows_pad, K, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_v_cache, n_heads, n_kv_heads, head_dim,
                                   max_len, dtype, stream, 0);
}

int samd_gemm_qkv_rope_norm_vt(const void *d_x, const float *d_ssq, const void *d_norm_weight, float eps, const void *d_W64, int32_t rows_pad, int32_t K,
                               const float *d_cs, const int32_t *d_cache_length, const int32_t *d_n, void *d_q_out, void *d_k_cache, void *d_vt_cache,
                               int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, int64_t max_len, int32_t dtype, void *stream) {
    return gemm_qkv_rope_norm_impl(d_x, d_ssq, d_norm_weight, eps, d_W64, rows_pad, K, d_cs, d_cache_length, d_n, d_q_out, d_k_cache, d_vt_cache, n_heads, n_kv_heads, head_dim,
                                   max_len, dtype, stream, 1);
}

int samd_gemm_skinny(const void *d_A, const void *d_W, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial,
                     void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_W || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || splits < 1 || splits > K / GEMM_KC || (splits == 1 ? !d_out : !d_partial) || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_skinny: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0) or null pointer"); return SAMD_E_INVALID;
    }
    const hipError_t e = gemm_dispatch<0>(dtype, rows_pad, dim3(N / GEMM_COLS, splits), (hipStream_t)stream, d_A, d_W, d_partial, splits == 1 ? d_out : nullptr, K, N,
                                          K / GEMM_KC, splits);
    if (e != hipSuccess) { samd_set_error("samd_gemm_skinny: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

/* samd_gemm_skinny over a GROUP-MAJOR matrix (samd_gemm_pack_groups of the plain [N][K] weight: the layout samd_gemm_cs_residual reads), so that
 * o_proj / down_proj keep one packed copy for every row bucket.  Same arguments, same results bit for bit (the lanes multiply the same values in
 * the same order; only where a wave finds its 16 columns differs). */
int samd_gemm_skinny_groups(const void *d_A, const void *d_Wg, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial,
                            void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_Wg || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || splits < 1 || splits > K / GEMM_KC || (splits == 1 ? !d_out : !d_partial) || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_skinny_groups: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0) or null pointer"); return SAMD_E_INVALID;
    }
    const hipError_t e = gemm_dispatch<0, true>(dtype, rows_pad, dim3(N / GEMM_COLS, splits), (hipStream_t)stream, d_A, d_Wg, d_partial, splits == 1 ? d_out : nullptr, K, N,
                                                K / GEMM_KC, splits);
    if (e != hipSuccess) { samd_set_error("samd_gemm_skinny_groups: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"

// ================================================================================================
// FP8 (OCP e4m3fn) weight-only projection: out[m][n] = scale[n] * sum_k A[m][k] * q[n][k], A in the model dtype, q one byte per weight,
// scale fp32 per output column (per output row of the HF weight).  Same grid, A staging, k permutation and MFMA sequence as k_gemm_skinny;
// only the weight load and a conversion differ, so the stream moves half the bytes.
//   PACKED LAYOUT (samd_gemm_pack_f8): block (tile t = 128 columns, chunk c = 256 k) is 32 KiB contiguous at ((t * K/256 + c) * 2048) uint4
//   units; unit b * 512 + tid holds q[128 t + 16 w + n][256 c + 64 b + 16 g .. +15] for tid = 64 w + 16 g + n -- in one 16-byte load the two
//   8-element vectors (j = 0, 1) that k_gemm_skinny loads separately.
// The bytes are widened in registers by v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1: every e4m3fn value is exact in fp16 and in bf16, so
// the MFMA sees the weights without error; the column scale is applied to the fp32 sums in the epilogue (one multiply per accumulator).
// DEPTH: 4 chunks of 32 KiB in flight = the fp16 kernel's 128 KiB per workgroup and its 64 weight VGPRs; at 64 rows DEPTH + 1 = 5 A buffers
// would take the whole 160 KiB of LDS, so that tile keeps 3 chunks in flight (4 buffers, 128 KiB).
// ================================================================================================
template <typename TT> struct F8Widen;
template <> struct F8Widen<GF16> {
    static __device__ __forceinline__ half8 cvt(unsigned w0, unsigned w1) {
        const auto a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
        const auto c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
        return __builtin_bit_cast(half8, (u32x4){__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, d)});
    }
};
template <> struct F8Widen<GBF16> {
    static __device__ __forceinline__ bf16x8 cvt(unsigned w0, unsigned w1) {
        const auto a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
        const auto c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
        return __builtin_bit_cast(bf16x8, (u32x4){__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, d)});
    }
};

// two A operands (16-byte units at a0, a1 of this lane's row) for each of the RT row tiles: the A-side read of the 8- and 4-bit streaming kernels
template <int RT>
__device__ __forceinline__ void gemm_read_a2(u32x4 (&r)[RT][2], uint32_t a0, uint32_t a1) {
    if constexpr (RT == 1)
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]) : "v"(a0), "v"(a1));
    else if constexpr (RT == 2)
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %4 offset:8192\n\tds_read_b128 %3, %5 offset:8192\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]) : "v"(a0), "v"(a1));
    else if constexpr (RT == 3)
        asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %6 offset:8192\n\tds_read_b128 %3, %7 offset:8192\n\t"
                     "ds_read_b128 %4, %6 offset:16384\n\tds_read_b128 %5, %7 offset:16384\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]) : "v"(a0), "v"(a1));
    else
        asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %8 offset:8192\n\tds_read_b128 %3, %9 offset:8192\n\t"
                     "ds_read_b128 %4, %8 offset:16384\n\tds_read_b128 %5, %9 offset:16384\n\tds_read_b128 %6, %8 offset:24576\n\t"
                     "ds_read_b128 %7, %9 offset:24576\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0][0]), "=&v"(r[0][1]), "=&v"(r[1][0]), "=&v"(r[1][1]), "=&v"(r[2][0]), "=&v"(r[2][1]), "=&v"(r[3][0]), "=&v"(r[3][1])
                     : "v"(a0), "v"(a1));
}

template <typename TT, int RT, int DEPTH>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_gemm_skinny_f8(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W8,
                                                                     const float *__restrict__ scale, float *__restrict__ partial,
                                                                     typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int n_splits) {
    typedef typename TT::elem E;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk (as k_gemm_skinny)
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 4 + XV;                     // memory operations per thread and chunk: 4 weight loads + the A staging
    constexpr size_t WCH = 32768, WU = 8192;       // bytes of one (tile, chunk) block; of one b row inside it
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    const int n0 = blockIdx.x * GEMM_COLS + 16 * w;
    const int split = blockIdx.y;
    const int c0 = (int)((long long)split * n_chunks / n_splits), c1 = (int)((long long)(split + 1) * n_chunks / n_splits);
    const char *wtile = reinterpret_cast<const char *>(W8) + (size_t)blockIdx.x * n_chunks * WCH;
    const uint32_t wlane = (uint32_t)tid * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];
    const float sc = scale[n0 + n];                // this lane's column; requested before the stream, used in the epilogue

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    // hand-issued nt weight loads, counted waits and bare barriers: see k_gemm_skinny
    u32x4 wr[DEPTH][4];
    auto load_wb = [&](u32x4 (&dst)[4], int c, int b) {
        const char *p = wtile + (size_t)c * WCH;
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst[b]) : "v"(wlane), "s"(p + WU * b) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)row * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4], int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    auto phase = [&](u32x4 (&cur)[4], int c, int buf) {
        gemm_wait_younger<DEPTH, PC>(c1 - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            gemm_read_a2<RT>(r, a0, a1);
            // the conversion is ordinary VALU code on the loaded registers: re-define them here, behind the counted wait (volatile asm keeps its
            // order), so that no conversion can be scheduled above the wait while the load is still in flight
            asm volatile("" : "+v"(cur[b]) : : "memory");
            const auto lo = F8Widen<TT>::cvt(cur[b][0], cur[b][1]), hi = F8Widen<TT>::cvt(cur[b][2], cur[b][3]);
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][0]), lo, acc[mt]);
                acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][1]), hi, acc[mt]);
            }
            if (RT >= 3 && c + DEPTH < c1) {       // 48 / 64 rows: refill per k block (see k_gemm_skinny)
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
            }
        }
        if (RT < 3 && c + DEPTH < c1) { load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
    if (c0 < c1) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c0 + d < c1) { load_w(wr[d], c0 + d); stage_x(c0 + d, d); }
        int buf = 0;
        for (int c = c0; c < c1; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < c1) { phase(wr[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // C layout of mfma_16x16: lane holds rows 4g + r of column n; the column scale goes on the fp32 sum, then ONE rounding to the model dtype
#pragma unroll
    for (int mt = 0; mt < RT; mt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 16 * mt + 4 * g + r;
            const float v = acc[mt][r] * sc;
            if (out) out[(size_t)m * N + n0 + n] = (E)v;
            else __hip_atomic_store(&partial[((size_t)split * R + m) * N + n0 + n], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// row-major [N][K] e4m3fn bytes -> the packed blocks of k_gemm_skinny_f8; one thread moves one 16-byte unit
__global__ __launch_bounds__(256) void k_gemm_pack_f8(const uint4 *__restrict__ W8, uint4 *__restrict__ out, int N, int K) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;          // destination unit
    const long long total = (long long)N * K / 16;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 11;                                          // 2048 units per 32 KiB block
    const int in = (int)(u & 2047), b = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks);
    const long long row = 128LL * t + 16 * w + n, col = 256LL * c + 64 * b + 16 * g;
    out[u] = W8[(row * K + col) / 16];
}

// the dynamic LDS of a streaming kernel with `depth` chunks in flight: depth + 1 A buffers of 16 rt rows
static constexpr int stream_lds(int depth, int rt) { return (depth + 1) * 16 * rt * GEMM_KC * 2; }

// one launch of a weight-only streaming kernel, dense or expert: dynamic LDS above 64 KiB is reserved once per kernel instantiation and device
template <auto KERN, int LDS, typename... A>
static hipError_t stream_launch(dim3 grid, hipStream_t st, A... args) {
    if constexpr (LDS > 65536) {
        static unsigned long long done = 0ull;                     // per-device (samd_common.h)
        const hipError_t attr = samd_reserve_lds((const void *)KERN, LDS, &done);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL(KERN, grid, dim3(64 * GEMM_WAVES), LDS, st, args...);
    return hipSuccess;
}

extern "C" {

int samd_gemm_pack_f8(const void *d_W8, void *d_out, int32_t N, int32_t K, void *stream) {
    if (!d_W8 || !d_out || d_W8 == d_out || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_gemm_pack_f8: needs N %% 128 == 0, K %% 256 == 0 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 16;
    hipLaunchKernelGGL(k_gemm_pack_f8, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W8, (uint4 *)d_out, N, K);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_skinny_f8(const void *d_A, const void *d_W8p, const float *d_scale, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial,
                        void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_W8p || !d_scale || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS || N % GEMM_COLS != 0 ||
        K < GEMM_KC || K % GEMM_KC != 0 || splits < 1 || splits > K / GEMM_KC || (splits == 1 ? !d_out : !d_partial) || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_skinny_f8: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0) or null pointer"); return SAMD_E_INVALID;
    }
    const dim3 grid(N / GEMM_COLS, splits);
    const hipStream_t st = (hipStream_t)stream;
    float *part = splits == 1 ? nullptr : d_partial;
    void *out = splits == 1 ? d_out : nullptr;
#define GO(TT, RT, D) e = stream_launch<k_gemm_skinny_f8<TT, RT, D>, stream_lds(D, RT)>(grid, st, (const typename TT::elem *)d_A, (const unsigned char *)d_W8p, \
        d_scale, part, (typename TT::elem *)out, K, N, K / GEMM_KC, splits)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1, 4); else if (rows_pad == 32) GO(TT, 2, 4); else if (rows_pad == 48) GO(TT, 3, 4); else GO(TT, 4, 3); } while (0)
    hipError_t e;
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_skinny_f8: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"

// ================================================================================================
// MXFP4 (OCP Microscaling: e2m1 elements, one e8m0 scale per 32 elements along k) weight-only projection:
// out[m][n] = sum_k A[m][k] * fp4(q[n][k]) * 2^(e8[n][k / 32] - 127), A in the model dtype.  Same grid, A staging and MFMA sequence as
// k_gemm_skinny_f8; the weight load, the conversion, the k permutation and the packed layout differ, and the stream moves 4.25 bits per weight.
//   PACKED LAYOUT (samd_gemm_pack_f4): block (tile t = 128 columns, chunk c = 256 k) is 17 KiB contiguous at (t * K/256 + c) * 17408 bytes:
//   16 KiB of elements, then 1 KiB of scales.  Element unit j * 512 + tid (16 bytes, j = 0, 1) holds the row-major bytes of
//   q[128 t + 16 w + n][256 c + 128 j + 32 g .. +31] for tid = 64 w + 16 g + n (byte i: low nibble k + 2 i, high nibble k + 2 i + 1) --
//   exactly one MX block, so a lane's unit converts with one scale.  Scale byte 16384 + 2 tid + j is e8[128 t + 16 w + n][8 c + 4 j + g]:
//   a lane fetches the two scales of its two units of a chunk in one 2-byte nt load, once per chunk (3 + XV memory operations per chunk).
// dword i of a unit is the 8-element MFMA operand k + 8 i .. + 7, so the A-side reads unit (16 j + 4 g + i) ^ n of row n.
// v_cvt_scalef32_pk_{f16,bf16}_fp4 widens two nibbles WITH the block scale (the float whose bits are e8 << 23): fp4 * 2^e is exact in the
// model dtype over the exponent range samd_hip/mxfp4.py admits, so the MFMA sees the weights without error and the epilogue applies nothing.
// DEPTH (chunks of 16 KiB + 1 KiB in flight per workgroup): 16 rows 8 (136 KiB; 9 A buffers = 72 KiB of LDS, two workgroups per CU),
// 32 rows 4 (5 buffers = 80 KiB, two workgroups per CU), 48 rows 5 (6 buffers = 144 KiB), 64 rows 3 (4 buffers = 128 KiB).  The only
// inline assembly beyond k_gemm_skinny_f8's forms is the 2-byte sibling of its weight load, global_load_ushort ... nt, for the scales.
// ================================================================================================
template <typename TT> struct F4Widen;
template <> struct F4Widen<GF16> {
    static __device__ __forceinline__ half8 cvt(unsigned w, float s) {
        const auto a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 1);
        const auto c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 3);
        return __builtin_bit_cast(half8, (u32x4){__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, d)});
    }
};
template <> struct F4Widen<GBF16> {
    static __device__ __forceinline__ bf16x8 cvt(unsigned w, float s) {
        const auto a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
        const auto c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
        return __builtin_bit_cast(bf16x8, (u32x4){__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, d)});
    }
};

// ================================================================================================
// INT4 (AWQ / GPTQ: unsigned 4-bit codes, one scale and one 4-bit zero point per 128 elements along k) weight-only projection:
// out[m][n] = sum_k A[m][k] * W[n][k], W[n][k] = rne_dtype((q[n][k] - z[n][k/128]) * s[n][k/128]), A and s in the model dtype
// (samd_hip/int4.py has the numeric contract).  Grid, A staging by LDS-DMA, A-side swizzle, counted waits, in-out load destinations and
// MFMA sequence are MXFP4's (one body, gemm_stream_w4 below); the weight block and the widening differ: integer arithmetic with a zero point and a scale that
// is no power of two, which v_cvt_scalef32_pk_*_fp4 cannot do.
//   PACKED LAYOUT (samd_gemm_pack_i4): block (tile t = 128 columns, chunk c = 256 k) is 17 KiB contiguous at (t * K/256 + c) * 17408 bytes:
//   16 KiB of elements, then 1 KiB of group data.  Element unit j * 512 + tid (16 bytes, j = 0, 1) holds the 32 codes
//   q[128 t + 16 w + n][256 c + 128 j + 32 g .. +31] for tid = 64 w + 16 g + n: all inside ONE 128-group, 2 c + j.  dword i of a unit
//   holds the codes k + 8 i .. + 7 (the 8-element MFMA operand, so the A-side reads unit (16 j + 4 g + i) ^ n of row n, as f4 does) with
//   the nibbles permuted: nibble p (bits 4p .. 4p + 3) is element 2 (p & 3) + (p >> 2), so that (x >> 4 i) & 0x000f000f is the k pair
//   (2 i, 2 i + 1) of the operand as two 16-bit lanes.  Group data: the 8 bytes at 16384 + 8 (16 w + n) are, as four 16-bit words,
//   s[row][2 c], s[row][2 c + 1], zb[row][2 c], zb[row][2 c + 1] -- s the scale's bits in the model dtype, zb the zero point pre-biased
//   as the dtype's bits of 1024 + z (fp16: 0x6400 | z) or 128 + z (bf16: 0x4300 | z).  A lane fetches them in one 8-byte nt load per chunk
//   (the four g lanes of a row read the same 8 bytes): 3 + XV memory operations per chunk, as f4.
// WIDENING, one rounding: fp16: 0x6400 | q is 1024 + q; v_pk_add_f16 by -(1024 + z) is exact (integers below 2048), v_pk_mul_f16 by s rounds
// once (fp16 denormals on).  bf16: (q << 16) | 0x43000000 is the fp32 128 + q; subtract the fp32 128 + z (exact), multiply by float(s)
// (exact in fp32: 5 x 8 significant bits), v_cvt_pk_bf16_f32 rounds once -- gfx950 has no packed bf16 arithmetic; this is the only new
// inline assembly besides the 8-byte sibling of the nt loads.  The conversion sits behind the counted wait, as f4's.
// DEPTH: MXFP4's table (16 rows 8, 32 rows 4, 48 rows 5, 64 rows 3): the group data costs one more VGPR per chunk in flight than
// f4's scales, and no instantiation spills (tests/test_int4_codeobject_cpu.py reads it from the code object's metadata).
// ================================================================================================
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

template <typename TT> struct I4Widen;
template <> struct I4Widen<GF16> {
    struct G { half2v s, zb; };
    static __device__ __forceinline__ G group(u32x2 gd, int j) {
        const unsigned s = (gd[0] >> (16 * j)) & 0xffffu, z = (gd[1] >> (16 * j)) & 0xffffu;
        return {__builtin_bit_cast(half2v, s | (s << 16)), __builtin_bit_cast(half2v, z | (z << 16))};
    }
    static __device__ __forceinline__ half8 cvt(unsigned x, G g) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const half2v q = __builtin_bit_cast(half2v, ((x >> (4 * i)) & 0x000f000fu) | 0x64006400u);      // (1024 + q_2i, 1024 + q_2i+1)
            r[i] = __builtin_bit_cast(unsigned, (q - g.zb) * g.s);
        }
        return __builtin_bit_cast(half8, r);
    }
};
template <> struct I4Widen<GBF16> {
    struct G { float s, zb; };
    static __device__ __forceinline__ G group(u32x2 gd, int j) {
        return {__builtin_bit_cast(float, (gd[0] >> (16 * j)) << 16), __builtin_bit_cast(float, (gd[1] >> (16 * j)) << 16)};
    }
    static __device__ __forceinline__ bf16x8 cvt(unsigned x, G g) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned t = x >> (4 * i);
            const float lo = __builtin_bit_cast(float, ((t << 16) & 0x000f0000u) | 0x43000000u);           // 128 + q_2i
            const float hi = __builtin_bit_cast(float, (t & 0x000f0000u) | 0x43000000u);                   // 128 + q_2i+1
            const float a = (lo - g.zb) * g.s, b = (hi - g.zb) * g.s;
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(a), "v"(b));
            r[i] = p;
        }
        return __builtin_bit_cast(bf16x8, r);
    }
};

// ================================================================================================
// THE SIDE of a weight-only streaming kernel: whose rows and whose weight tile a workgroup works on, and where its sums go.  A kernel is a
// weight stream (one body per format: gemm_stream_w4, gemm_stream_i8) times a side, chosen by `if constexpr` inside the body.
//   SIDE_DENSE   rows 0 .. R - 1 of A, weight tile blockIdx.x, the chunk range [c0, c1) of split blockIdx.y, and stream_store_dense: the
//                rounded sum (splits == 1) or the split's fp32 partial.
//   SIDE_EXPERT  one active expert's share of a gathered projection (the mixture-of-experts sections below have the calls and the routing
//                workspace).  The grid's y dimension is the shape's upper bound of active experts, min(E, rows * k); a workgroup whose
//                slot is >= ws[0], the count the router left on the device, exits at once (moe_side_idle: uniform, before any barrier).  moe_side_open
//                reads the slot's expert and entry count (clamped to the row tile) and copies its list of entries p = row * k + slot into
//                static LDS; tile rows past the count repeat entry 0, so every staged row is a valid one.  The caller's __syncthreads()
//                follows -- left to the caller so that a body can stage more static LDS under the same barrier, as moe8_expert_gemm does
//                with its scales.  moe_side_row gives a thread the XV source rows of its A staging units (srow: p / k of h for gate|up, p
//                itself of act for down): the gather is an indirection on the LDS-DMA's source address, no copy.  The chunk range is the
//                whole of K: no split-K, no atomics.  moe_side_store is the epilogue; rows >= cnt are not stored.  GU: waves 4-7 hold the
//                up columns that waves 0-3's gate columns meet; they pass through LDS (the A tiles are dead by then) and act[p][I] gets
//                HF's act_fn(gate) * up with its roundings in the model dtype: gate, up, silu(gate) and the product each rounded once (as
//                k_gemm_skinny EPI 1 / k_silu_mul).  Otherwise y[p][N] gets the sum rounded once.
//   SIDE_WIDE    the expert side over the wide workspace (one-pass prefill): the slot is a TILE of 64 entries, ws[0] the tile count, and
//                the tile's record {expert, first entry, entries} names the expert and its part of the entry array.
// ================================================================================================
enum { SIDE_DENSE, SIDE_EXPERT, SIDE_WIDE };

#define MOE_MAX_E 256
#define MOE_MAX_K 8
#define MOE_MAX_ROWS 64
#define MOE_WS_ACTIVE 16
#define MOE_WS_COUNT (MOE_WS_ACTIVE + MOE_MAX_E)
#define MOE_WS_LIST (MOE_WS_COUNT + MOE_MAX_E)
#define MOE_WS_INTS (MOE_WS_LIST + MOE_MAX_E * MOE_MAX_ROWS)
#define MOE_WS_Y_OFF (((MOE_WS_INTS * 4 + 255) / 256) * 256)
// the wide calls' routing workspace (samd_moe_wide_*, at the end of the mixture-of-experts sections): fixed word offsets, so that the
// expert side reads a tile record without knowing the shape
#define MOEW_MAX_ROWS 4096
#define MOEW_TILE_INTS 3
#define MOEW_MAX_TILES (MOE_MAX_E + MOEW_MAX_ROWS * MOE_MAX_K / MOE_MAX_ROWS)
#define MOEW_WS_ACTIVE 16
#define MOEW_WS_COUNT (MOEW_WS_ACTIVE + MOE_MAX_E)
#define MOEW_WS_OFFSET (MOEW_WS_COUNT + MOE_MAX_E)
#define MOEW_WS_TILE (MOEW_WS_OFFSET + MOE_MAX_E)
#define MOEW_WS_ENTRY (MOEW_WS_TILE + MOEW_TILE_INTS * MOEW_MAX_TILES)

// the workgroup's list of entries, in static LDS
__device__ __forceinline__ int *moe_side_list() {
    __shared__ int lst[MOE_MAX_ROWS];
    return lst;
}

// no work for this slot (uniform): the caller returns at once.  (Kept apart from moe_side_open so that the exit is a plain branch of the kernel.)
__device__ __forceinline__ bool moe_side_idle(const int *ws) { return (int)blockIdx.y >= ws[0]; }

// the slot's expert, its entry count (<= R) and the list fill; the caller's barrier follows.  (The helpers return values, not references:
// what they compute then folds into the kernel as if written there, and the code objects stay those of the hand-written copies.)
struct MoeSlot { int expert, cnt; };
template <int R, bool WIDE>
__device__ __forceinline__ MoeSlot moe_side_open(const int *ws) {
    int *lst = moe_side_list();
    const int tid = threadIdx.x, slot_a = blockIdx.y;
    const int *rec = ws + MOEW_WS_TILE + MOEW_TILE_INTS * slot_a;     // WIDE: the tile's record {expert, first entry, entries}
    const int expert = WIDE ? rec[0] : ws[MOE_WS_ACTIVE + slot_a];
    int cnt = WIDE ? rec[2] : ws[MOE_WS_COUNT + slot_a];
    cnt = cnt > R ? R : cnt;
    const int *ent = WIDE ? ws + MOEW_WS_ENTRY + rec[1] : ws + MOE_WS_LIST + MOE_MAX_ROWS * slot_a;
    if (tid < MOE_MAX_ROWS) lst[tid] = ent[tid < cnt ? tid : 0];
    return {expert, cnt};
}

// source row i of this thread's A staging units: tile row r = entry r of the expert's list (rows past the count: entry 0 again)
template <bool GU>
__device__ __forceinline__ int moe_side_row(int i, int top_k) {
    const int tid = threadIdx.x;
    const int p = moe_side_list()[(tid >> 5) + 16 * i];
    return GU ? p / top_k : p;
}

// C layout of mfma_16x16: lane (w, n, g -- the caller's own values, so that its expressions stay shared) holds rows 4g + r of column n.
// ex: the dynamic LDS, [R][64] up values
template <typename TT, int RT, bool GU>
__device__ __forceinline__ void moe_side_store(const floatx4 (&acc)[RT], int cnt, typename TT::elem *out, int N, float *ex, int w, int n, int g) {
    typedef typename TT::elem E;
    const int *lst = moe_side_list();
    if constexpr (GU) {
        __syncthreads();
        if (w >= 4) {
#pragma unroll
            for (int mt = 0; mt < RT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) ex[(16 * mt + 4 * g + r) * 64 + 16 * (w - 4) + n] = acc[mt][r];
        }
        __syncthreads();
        if (w < 4) {
#pragma unroll
            for (int mt = 0; mt < RT; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int m = 16 * mt + 4 * g + r;
                    if (m >= cnt) continue;
                    const float gf = (float)(E)acc[mt][r], uf = (float)(E)ex[m * 64 + 16 * w + n];
                    const E sv = (E)(gf / (1.f + __expf(-gf)));
                    out[(size_t)lst[m] * (N / 2) + blockIdx.x * 64 + 16 * w + n] = (E)((float)sv * uf);
                }
        }
    } else {
        const int n0 = blockIdx.x * GEMM_COLS + 16 * w;
#pragma unroll
        for (int mt = 0; mt < RT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = 16 * mt + 4 * g + r;
                if (m < cnt) out[(size_t)lst[m] * N + n0 + n] = (E)acc[mt][r];
            }
    }
}

// the dense side's store: the scales went in with the widening, so ONE rounding and nothing else; a split stores its fp32 partial
template <typename TT, int RT>
__device__ __forceinline__ void stream_store_dense(const floatx4 (&acc)[RT], float *partial, typename TT::elem *out, int N, int w, int n, int g) {
    typedef typename TT::elem E;
    const int n0 = blockIdx.x * GEMM_COLS + 16 * w, split = blockIdx.y;
#pragma unroll
    for (int mt = 0; mt < RT; mt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 16 * mt + 4 * g + r;
            const float v = acc[mt][r];
            if (out) out[(size_t)m * N + n0 + n] = (E)v;
            else __hip_atomic_store(&partial[((size_t)split * (16 * RT) + m) * N + n0 + n], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ================================================================================================
// The 4-bit streaming body shared by MXFP4 and INT4.  Both formats stream 17 KiB (tile, chunk) blocks -- 16 KiB of elements, then 1 KiB of
// per-chunk side data -- over the grid, the LDS-DMA A staging, the A-side swizzle and the MFMA order of k_gemm_skinny_f8.  A format is a
// small policy: the type of a lane's side data (side_t), its byte offset behind the elements (slane), the ONE nt load that fetches it
// (load_side), and the widening (group: the side data of unit j; cvt: one dword of 8 codes -> one MFMA operand).
// ================================================================================================
struct W4Mx {                                      // side data: the chunk's two e8m0 codes of this lane, bits 0-7 unit 0, bits 8-15 unit 1
    typedef unsigned side_t;
    static constexpr bool mx = true;
    static __device__ __forceinline__ uint32_t slane(int tid, int, int) { return (uint32_t)tid * 2; }
    static __device__ __forceinline__ void load_side(side_t &dst, uint32_t slane, const char *p) {
        asm volatile("global_load_ushort %0, %1, %2 nt" : "+v"(dst) : "v"(slane), "s"(p) : "memory");
    }
    template <typename TT> static __device__ __forceinline__ float group(side_t e8s, int j) {
        return __builtin_bit_cast(float, ((e8s >> (8 * j)) & 0xffu) << 23);                     // 2^(e8 - 127)
    }
    template <typename TT> static __device__ __forceinline__ auto cvt(unsigned x, float sc) { return F4Widen<TT>::cvt(x, sc); }
};
struct W4Int {                                     // side data: the group data of this lane's row, {s0 | s1 << 16, zb0 | zb1 << 16}
    typedef u32x2 side_t;
    static constexpr bool mx = false;
    static __device__ __forceinline__ uint32_t slane(int, int w, int n) { return (uint32_t)(16 * w + n) * 8; }
    static __device__ __forceinline__ void load_side(side_t &dst, uint32_t slane, const char *p) {
        asm volatile("global_load_dwordx2 %0, %1, %2 nt" : "+v"(dst) : "v"(slane), "s"(p) : "memory");
    }
    template <typename TT> static __device__ __forceinline__ auto group(side_t gd, int j) { return I4Widen<TT>::group(gd, j); }
    template <typename TT> static __device__ __forceinline__ auto cvt(unsigned x, typename I4Widen<TT>::G g) { return I4Widen<TT>::cvt(x, g); }
};

// gemm_wait_younger for pipelines deeper than 4 chunks: wait until at most min(younger, DEPTH - 1) * PC memory operations are outstanding
template <int DEPTH, int PC>
__device__ __forceinline__ void gemm_wait_younger_deep(int younger) {
    static_assert(DEPTH <= 8 && (DEPTH - 1) * PC <= 63, "vmcnt is a 6-bit counter");
#define SAMD_WAIT_IF(i) if (DEPTH > i && younger >= i) { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(DEPTH > i ? i * PC : 0) : "memory"); return; }
    SAMD_WAIT_IF(7) SAMD_WAIT_IF(6) SAMD_WAIT_IF(5) SAMD_WAIT_IF(4) SAMD_WAIT_IF(3) SAMD_WAIT_IF(2) SAMD_WAIT_IF(1)
#undef SAMD_WAIT_IF
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
}

// THE PIPELINE (explained here for every weight-only stream with in-out destinations: gemm_stream_i8, moe_expert_gemm, moe8_expert_gemm
// and k_gemm_skinny_f8b point here).
//   Hand-issued nt element and side-data loads, counted waits and bare barriers: see k_gemm_skinny.  3 + XV memory operations per lane and
//   chunk: 2 element loads, 1 side-data load, the A staging.
//   In-out destinations: the destination registers are defined once, up front, and every load is an in-out ("+v") of that value.  A load
//   that a short split (or a short expert stream) skips then leaves the SAME register behind, so the compiler has no two values to merge
//   with a copy -- a v_mov of a register whose load is still in flight would move stale bits and leave the landing load to overwrite
//   whatever lives there by then.  This fault was met once, with a split whose prologue skipped a load.
//   Re-definition behind the wait: the widening is ordinary VALU code on the loaded registers, so they are re-defined behind the counted
//   wait (volatile asm keeps its order) and no conversion can be scheduled above the wait while the load is still in flight.
//   Per-unit refill at 48 / 64 rows: a unit's registers are loaded again as soon as its MFMAs have read them, with that unit's share of
//   the A staging, instead of all at the end of the phase (see k_gemm_skinny); the side data follows its last use.
// F: the weight policy.  SIDE, GU: see THE SIDE; ws and `aux` = top_k belong to the expert sides, partial and `aux` = n_splits to the dense one.
template <typename F, typename TT, int RT, int DEPTH, int SIDE, bool GU = false>
__device__ __forceinline__ void gemm_stream_w4(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W4, const int *__restrict__ ws,
                                               float *__restrict__ partial, typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int aux) {
    typedef typename TT::elem E;
    typedef typename F::side_t side_t;
    constexpr bool MOE = SIDE != SIDE_DENSE;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk (as k_gemm_skinny)
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 3 + XV;                     // memory operations per thread and chunk: 2 element loads + 1 side-data load + the A staging
    constexpr size_t WCH = 17408, WU = 8192, WS = 16384;   // bytes of one (tile, chunk) block; of one j row inside it; offset of its side data
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    // the side: the weight tile, the chunk range [c0, c1) and the source row of tile row r (expert sides: srow)
    MoeSlot slot = {0, 0};
    int srow[XV];
    if constexpr (MOE) {
        if (moe_side_idle(ws)) return;
        slot = moe_side_open<R, SIDE == SIDE_WIDE>(ws);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XV; i++) srow[i] = moe_side_row<GU>(i, aux);
    }
    const int split = blockIdx.y;
    const int c0 = MOE ? 0 : (int)((long long)split * n_chunks / aux), c1 = MOE ? n_chunks : (int)((long long)(split + 1) * n_chunks / aux);
    const char *wtile = reinterpret_cast<const char *>(W4) + (MOE ? (size_t)slot.expert * (N / GEMM_COLS) + blockIdx.x : (size_t)blockIdx.x) * n_chunks * WCH;
    const uint32_t wlane = (uint32_t)tid * 16, slane = F::slane(tid, w, n);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    u32x4 wr[DEPTH][2];
    side_t sd[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; d++) asm volatile("" : "=v"(wr[d][0]), "=v"(wr[d][1]), "=v"(sd[d]));
    auto load_wj = [&](u32x4 (&dst)[2], int c, int j) {
        const char *p = wtile + (size_t)c * WCH;
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "+v"(dst[j]) : "v"(wlane), "s"(p + WU * j) : "memory");
    };
    auto load_s = [&](side_t &dst, int c) { F::load_side(dst, slane, wtile + (size_t)c * WCH + WS); };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)(MOE ? srow[i] : row) * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[2], side_t &sdst, int c) {
        load_wj(dst, c, 0); load_wj(dst, c, 1); load_s(sdst, c);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    auto phase = [&](u32x4 (&cur)[2], side_t &cs, int c, int buf) {
        gemm_wait_younger_deep<DEPTH, PC>(c1 - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
        asm volatile("" : "+v"(cs) : : "memory");
        const side_t side = cs;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            asm volatile("" : "+v"(cur[j]) : : "memory");
            const auto grp = F::template group<TT>(side, j);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int u = 16 * j + 4 * g + 2 * h;
                const uint32_t a0 = xbase + (uint32_t)(u ^ n) * 16, a1 = xbase + (uint32_t)((u + 1) ^ n) * 16;
                u32x4 r[RT][2];
                gemm_read_a2<RT>(r, a0, a1);
                const auto lo = F::template cvt<TT>(cur[j][2 * h], grp), hi = F::template cvt<TT>(cur[j][2 * h + 1], grp);
#pragma unroll
                for (int mt = 0; mt < RT; mt++) {
                    acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][0]), lo, acc[mt]);
                    acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][1]), hi, acc[mt]);
                }
            }
            if (RT >= 3 && c + DEPTH < c1) {       // 48 / 64 rows: refill per unit (see k_gemm_skinny)
                load_wj(cur, c + DEPTH, j);
                if (j == 1) load_s(cs, c + DEPTH);
#pragma unroll
                for (int i = 2 * j; i < 2 * j + 2; i++)
                    if (i < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, i);
            }
        }
        if (RT < 3 && c + DEPTH < c1) { load_w(cur, cs, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
    if (MOE || c0 < c1) {                          // (a dense split may be empty; an expert's stream is not)
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c0 + d < c1) { load_w(wr[d], sd[d], c0 + d); stage_x(c0 + d, d); }
        int buf = 0;
        for (int c = c0; c < c1; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < c1) { phase(wr[d], sd[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // block scales / scale and zero point went in with the widening: the sums are final
    if constexpr (MOE) moe_side_store<TT, RT, GU>(acc, slot.cnt, out, N, reinterpret_cast<float *>(gemm_lds), w, n, g);
    else stream_store_dense<TT, RT>(acc, partial, out, N, w, n, g);
}

template <typename TT, int RT, int DEPTH>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_gemm_skinny_f4(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W4,
                                                                     float *__restrict__ partial, typename TT::elem *__restrict__ out, int K, int N,
                                                                     int n_chunks, int n_splits) {
    gemm_stream_w4<W4Mx, TT, RT, DEPTH, SIDE_DENSE>(A, W4, nullptr, partial, out, K, N, n_chunks, n_splits);
}

template <typename TT, int RT, int DEPTH>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_gemm_skinny_i4(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W4,
                                                                     float *__restrict__ partial, typename TT::elem *__restrict__ out, int K, int N,
                                                                     int n_chunks, int n_splits) {
    gemm_stream_w4<W4Int, TT, RT, DEPTH, SIDE_DENSE>(A, W4, nullptr, partial, out, K, N, n_chunks, n_splits);
}

// row-major q [N][K/2] bytes + e8 [N][K/32] codes -> the packed blocks of k_gemm_skinny_f4; one thread moves one 16-byte unit and its scale
__global__ __launch_bounds__(256) void k_gemm_pack_f4(const uint4 *__restrict__ q, const unsigned char *__restrict__ e8, unsigned char *__restrict__ out,
                                                      int N, int K) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;          // element unit = MX block
    const long long total = (long long)N * K / 32;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 10;                                          // 1024 element units per block
    const int in = (int)(u & 1023), j = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks);
    const long long row = 128LL * t + 16 * w + n, mxb = 8LL * c + 4 * j + g;      // weight row; its MX block along k
    unsigned char *dst = out + blk * 17408;
    reinterpret_cast<uint4 *>(dst)[in] = q[row * (K / 32) + mxb];
    dst[16384 + 2 * tid + j] = e8[row * (K / 32) + mxb];
}

// row-major q [N][K/2] bytes, z [N][K/128] bytes, s [N][K/128] 16-bit words -> the packed blocks of k_gemm_skinny_i4; one thread moves one
// 16-byte unit (nibbles permuted inside each dword), the g == 0 thread of a row also its half of the row's group data
__global__ __launch_bounds__(256) void k_gemm_pack_i4(const uint4 *__restrict__ q, const unsigned char *__restrict__ z, const unsigned short *__restrict__ s,
                                                      unsigned char *__restrict__ out, int N, int K, unsigned zbias) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;          // element unit: 32 codes of one row
    const long long total = (long long)N * K / 32;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 10;                                          // 1024 element units per block
    const int in = (int)(u & 1023), j = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks);
    const long long row = 128LL * t + 16 * w + n, ub = 8LL * c + 4 * j + g;       // weight row; its 32-code unit along k
    unsigned char *dst = out + blk * 17408;
    const uint4 v = q[row * (K / 32) + ub];
    const unsigned src[4] = {v.x, v.y, v.z, v.w};
    unsigned d[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        unsigned o = 0;
#pragma unroll
        for (int p = 0; p < 8; p++) o |= ((src[i] >> (4 * (2 * (p & 3) + (p >> 2)))) & 15u) << (4 * p);
        d[i] = o;
    }
    reinterpret_cast<uint4 *>(dst)[in] = make_uint4(d[0], d[1], d[2], d[3]);
    if (g == 0) {
        const long long grp = row * (K / 128) + 2 * c + j;
        unsigned short *gdst = reinterpret_cast<unsigned short *>(dst + 16384 + 8 * (16 * w + n));
        gdst[j] = s[grp];
        gdst[2 + j] = (unsigned short)(zbias | (z[grp] & 15u));
    }
}

// the dense 4-bit kernels and their DEPTH row (16 / 32 / 48 / 64 rows), one for both formats
template <typename F> struct SkinnyW4 {
    static constexpr int depth(int rt) { return rt == 1 ? 8 : rt == 2 ? 4 : rt == 3 ? 5 : 3; }
    template <typename TT, int RT> static constexpr auto kern() { return F::mx ? k_gemm_skinny_f4<TT, RT, depth(RT)> : k_gemm_skinny_i4<TT, RT, depth(RT)>; }
};

// samd_gemm_skinny_f4 / _i4 / _i8: the checks, the grid and the row-tile / dtype dispatch; D names the format's kernels and its DEPTH row
template <typename D>
static int gemm_skinny_q_call(const char *fn, const void *d_A, const void *d_Wp, int rows_pad, int N, int K, int splits, float *d_partial, void *d_out, int dtype,
                              void *stream) {
    if (!d_A || !d_Wp || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS || N % GEMM_COLS != 0 ||
        K < GEMM_KC || K % GEMM_KC != 0 || splits < 1 || splits > K / GEMM_KC || (splits == 1 ? !d_out : !d_partial) || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("%s: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0) or null pointer", fn); return SAMD_E_INVALID;
    }
    const dim3 grid(N / GEMM_COLS, splits);
    const hipStream_t st = (hipStream_t)stream;
    float *part = splits == 1 ? nullptr : d_partial;
    void *out = splits == 1 ? d_out : nullptr;
#define GO(TT, RT) e = stream_launch<D::template kern<TT, RT>(), stream_lds(D::depth(RT), RT)>( \
        grid, st, (const typename TT::elem *)d_A, (const unsigned char *)d_Wp, part, (typename TT::elem *)out, K, N, K / GEMM_KC, splits)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1); else if (rows_pad == 32) GO(TT, 2); else if (rows_pad == 48) GO(TT, 3); else GO(TT, 4); } while (0)
    hipError_t e;
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("%s: %s", fn, hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

extern "C" {

int samd_gemm_pack_f4(const void *d_q, const void *d_e8, void *d_out, int32_t N, int32_t K, void *stream) {
    if (!d_q || !d_e8 || !d_out || d_q == d_out || d_e8 == d_out || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_gemm_pack_f4: needs N %% 128 == 0, K %% 256 == 0 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 32;
    hipLaunchKernelGGL(k_gemm_pack_f4, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_q,
                       (const unsigned char *)d_e8, (unsigned char *)d_out, N, K);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_pack_i4(const void *d_q, const void *d_z, const void *d_s, void *d_out, int32_t N, int32_t K, int32_t dtype, void *stream) {
    if (!d_q || !d_z || !d_s || !d_out || d_q == d_out || d_z == d_out || d_s == d_out || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_pack_i4: needs N %% 128 == 0, K %% 256 == 0, dtype fp16 or bf16 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 32;
    hipLaunchKernelGGL(k_gemm_pack_i4, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_q,
                       (const unsigned char *)d_z, (const unsigned short *)d_s, (unsigned char *)d_out, N, K, dtype == SAMD_F16 ? 0x6400u : 0x4300u);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_skinny_f4(const void *d_A, const void *d_W4p, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial, void *d_out,
                        int32_t dtype, void *stream) {
    return gemm_skinny_q_call<SkinnyW4<W4Mx>>("samd_gemm_skinny_f4", d_A, d_W4p, rows_pad, N, K, splits, d_partial, d_out, dtype, stream);
}

int samd_gemm_skinny_i4(const void *d_A, const void *d_W4p, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial, void *d_out,
                        int32_t dtype, void *stream) {
    return gemm_skinny_q_call<SkinnyW4<W4Int>>("samd_gemm_skinny_i4", d_A, d_W4p, rows_pad, N, K, splits, d_partial, d_out, dtype, stream);
}

}  // extern "C"

// ================================================================================================
// INT8 (GPTQ: unsigned 8-bit codes, one scale and one 8-bit zero point per 128 elements along k) weight-only projection:
// out[m][n] = sum_k A[m][k] * W[n][k], W[n][k] = rne_dtype((q[n][k] - z[n][k/128]) * s[n][k/128]), A and s in the model dtype
// (samd_hip/int8.py has the numeric contract).  The stream is k_gemm_skinny_f8's: grid, 32 KiB of codes per (tile, chunk), four hand-issued
// nt 16-byte loads per lane and chunk, A staging by LDS-DMA with the A-side swizzle, counted waits, the per-k-block refill at 48 / 64 rows.
// The group data is k_gemm_skinny_i4's: one 8-byte nt load per lane and chunk, in-out load destinations defined once.
//   PACKED LAYOUT (samd_gemm_pack_i8): block (tile t = 128 columns, chunk c = 256 k) is 33 KiB contiguous at (t * K/256 + c) * 33792 bytes:
//   32 KiB of codes, then 1 KiB of group data.  Code unit b * 512 + tid (16 bytes, b = 0..3) holds the 16 codes
//   q[128 t + 16 w + n][256 c + 64 b + 16 g .. +15] for tid = 64 w + 16 g + n, in k order, one byte each (samd_gemm_pack_f8's unit): all
//   inside ONE 128-group, 2 c + (b >> 1).  Group data: the 8 bytes at 32768 + 8 (16 w + n) are, as four 16-bit words, s[row][2 c],
//   s[row][2 c + 1], zb[row][2 c], zb[row][2 c + 1] -- s the scale's bits in the model dtype, zb the zero point in the form the dtype's
//   widening subtracts: fp16 the bits of 1024 + z (0x6400 | z), bf16 the bits of z itself (0..255 are exact in bf16's 8 significant bits).
//   The four g lanes of a row read the same 8 bytes: 5 + XV memory operations per lane and chunk.
// WIDENING, one rounding: fp16: a byte under 0x64 is the fp16 1024 + q (one v_perm_b32 per k pair); v_pk_add_f16 by -(1024 + z) is exact
// (integers below 2048), v_pk_mul_f16 by s rounds once (fp16 denormals on).  bf16: v_cvt_f32_ubyte{0..3} gives q exactly in fp32; minus
// float(z) is exact, times float(s) is exact in fp32 (9 x 8 significant bits), v_cvt_pk_bf16_f32 rounds once.  The library builds with
// -ffp-contract=off, so (q - z) * s stays two operations.  The conversion sits behind the counted wait, as f8's.
// DEPTH: k_gemm_skinny_f8's table (4 / 4 / 4 / 3 chunks in flight at 16 / 32 / 48 / 64 rows): 16 weight VGPRs + 2 of group data per chunk in
// flight; no instantiation spills (tests/test_int8_codeobject_cpu.py reads it from the code object's metadata).
// ================================================================================================
typedef float float2v __attribute__((ext_vector_type(2)));

template <typename TT> struct I8Widen;
template <> struct I8Widen<GF16> {
    struct G { half2v s, zb; };
    static __device__ __forceinline__ G group(u32x2 gd, int j) {
        const unsigned s = (gd[0] >> (16 * j)) & 0xffffu, z = (gd[1] >> (16 * j)) & 0xffffu;
        return {__builtin_bit_cast(half2v, s | (s << 16)), __builtin_bit_cast(half2v, z | (z << 16))};
    }
    // 8 codes (two dwords, k order) -> the 8-element MFMA operand
    static __device__ __forceinline__ half8 cvt(unsigned x0, unsigned x1, G g) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned x = i < 2 ? x0 : x1;
            // v_perm_b32: selector bytes 0..3 take bytes of the second source, 4..7 of the first: (0x64, q_2i+1, 0x64, q_2i) from the high byte down
            const unsigned p = __builtin_amdgcn_perm(0x64646464u, x, (i & 1) ? 0x04030402u : 0x04010400u);
            r[i] = __builtin_bit_cast(unsigned, (__builtin_bit_cast(half2v, p) - g.zb) * g.s);              // (1024 + q) - (1024 + z), then ONE rounding
        }
        return __builtin_bit_cast(half8, r);
    }
};
template <> struct I8Widen<GBF16> {
    struct G { float s, zb; };
    static __device__ __forceinline__ G group(u32x2 gd, int j) {
        return {__builtin_bit_cast(float, (gd[0] >> (16 * j)) << 16), __builtin_bit_cast(float, (gd[1] >> (16 * j)) << 16)};
    }
    static __device__ __forceinline__ bf16x8 cvt(unsigned x0, unsigned x1, G g) {
        u32x4 r;
        const float2v zz = {g.zb, g.zb}, ss = {g.s, g.s};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned x = (i < 2 ? x0 : x1) >> (16 * (i & 1));
            const float2v q = {(float)(x & 0xffu), (float)((x >> 8) & 0xffu)};                               // v_cvt_f32_ubyte*: exact
            const float2v v = (q - zz) * ss;                                                                // both exact in fp32; not fused
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v[0]), "v"(v[1]));
            r[i] = p;
        }
        return __builtin_bit_cast(bf16x8, r);
    }
};

// The INT8 streaming body, dense and expert: THE PIPELINE of gemm_stream_w4 (in-out destinations defined once, re-definition behind the
// counted wait, per-k-block refill at 48 / 64 rows) over four code loads and one group-data load per chunk, and the same sides (THE SIDE).
// A body of its own beside the 4-bit one because the PHASE differs, not the side: four code loads per chunk where the 4-bit stream has
// two, one A unit pair per load where that one has two, another A-side unit order and another refill cadence.
template <typename TT, int RT, int DEPTH, int SIDE, bool GU = false>
__device__ __forceinline__ void gemm_stream_i8(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W8, const int *__restrict__ ws,
                                               float *__restrict__ partial, typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int aux) {
    typedef typename TT::elem E;
    constexpr bool MOE = SIDE != SIDE_DENSE;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk (as k_gemm_skinny)
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 5 + XV;                     // memory operations per thread and chunk: 4 code loads + 1 group-data load + the A staging
    constexpr size_t WCH = 33792, WU = 8192, WS = 32768;   // bytes of one (tile, chunk) block; of one b row inside it; offset of its group data
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    // the side, as in gemm_stream_w4
    MoeSlot slot = {0, 0};
    int srow[XV];
    if constexpr (MOE) {
        if (moe_side_idle(ws)) return;
        slot = moe_side_open<R, SIDE == SIDE_WIDE>(ws);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XV; i++) srow[i] = moe_side_row<GU>(i, aux);
    }
    const int split = blockIdx.y;
    const int c0 = MOE ? 0 : (int)((long long)split * n_chunks / aux), c1 = MOE ? n_chunks : (int)((long long)(split + 1) * n_chunks / aux);
    const char *wtile = reinterpret_cast<const char *>(W8) + (MOE ? (size_t)slot.expert * (N / GEMM_COLS) + blockIdx.x : (size_t)blockIdx.x) * n_chunks * WCH;
    const uint32_t wlane = (uint32_t)tid * 16, slane = (uint32_t)(16 * w + n) * 8;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    u32x4 wr[DEPTH][4];
    u32x2 gs[DEPTH];                               // the chunk's group data of this lane's row: {s0 | s1 << 16, zb0 | zb1 << 16}
#pragma unroll
    for (int d = 0; d < DEPTH; d++) asm volatile("" : "=v"(wr[d][0]), "=v"(wr[d][1]), "=v"(wr[d][2]), "=v"(wr[d][3]), "=v"(gs[d]));
    auto load_wb = [&](u32x4 (&dst)[4], int c, int b) {
        const char *p = wtile + (size_t)c * WCH;
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "+v"(dst[b]) : "v"(wlane), "s"(p + WU * b) : "memory");
    };
    auto load_s = [&](u32x2 &dst, int c) {
        const char *p = wtile + (size_t)c * WCH + WS;
        asm volatile("global_load_dwordx2 %0, %1, %2 nt" : "+v"(dst) : "v"(slane), "s"(p) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)(MOE ? srow[i] : row) * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4], u32x2 &sdst, int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
        load_s(sdst, c);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    auto phase = [&](u32x4 (&cur)[4], u32x2 &cs, int c, int buf) {
        gemm_wait_younger_deep<DEPTH, PC>(c1 - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
        asm volatile("" : "+v"(cs) : : "memory");
        const u32x2 gd = cs;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            gemm_read_a2<RT>(r, a0, a1);
            asm volatile("" : "+v"(cur[b]) : : "memory");
            const auto grp = I8Widen<TT>::group(gd, b >> 1);
            const auto lo = I8Widen<TT>::cvt(cur[b][0], cur[b][1], grp), hi = I8Widen<TT>::cvt(cur[b][2], cur[b][3], grp);
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][0]), lo, acc[mt]);
                acc[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][1]), hi, acc[mt]);
            }
            if (RT >= 3 && c + DEPTH < c1) {       // 48 / 64 rows: refill per k block (see k_gemm_skinny)
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
                if (b == 3) load_s(cs, c + DEPTH);                 // (after the group data's last use)
            }
        }
        if (RT < 3 && c + DEPTH < c1) { load_w(cur, cs, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
    if (MOE || c0 < c1) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c0 + d < c1) { load_w(wr[d], gs[d], c0 + d); stage_x(c0 + d, d); }
        int buf = 0;
        for (int c = c0; c < c1; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < c1) { phase(wr[d], gs[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // scale and zero point went in with the widening: the sums are final
    if constexpr (MOE) moe_side_store<TT, RT, GU>(acc, slot.cnt, out, N, reinterpret_cast<float *>(gemm_lds), w, n, g);
    else stream_store_dense<TT, RT>(acc, partial, out, N, w, n, g);
}

template <typename TT, int RT, int DEPTH>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_gemm_skinny_i8(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W8,
                                                                     float *__restrict__ partial, typename TT::elem *__restrict__ out, int K, int N,
                                                                     int n_chunks, int n_splits) {
    gemm_stream_i8<TT, RT, DEPTH, SIDE_DENSE>(A, W8, nullptr, partial, out, K, N, n_chunks, n_splits);
}

// row-major q [N][K] bytes, z [N][K/128] bytes, s [N][K/128] 16-bit words -> the packed blocks of k_gemm_skinny_i8; one thread moves one
// 16-byte unit (as k_gemm_pack_f8), the g == 0 thread of k blocks 0 and 2 also that half of its row's group data
__global__ __launch_bounds__(256) void k_gemm_pack_i8(const uint4 *__restrict__ q, const unsigned char *__restrict__ z, const unsigned short *__restrict__ s,
                                                      unsigned char *__restrict__ out, int N, int K, int bf16) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;          // code unit: 16 codes of one row
    const long long total = (long long)N * K / 16;
    if (u >= total) return;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 11;                                          // 2048 code units per block
    const int in = (int)(u & 2047), b = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks);
    const long long row = 128LL * t + 16 * w + n, col = 256LL * c + 64 * b + 16 * g;
    unsigned char *dst = out + blk * 33792;
    reinterpret_cast<uint4 *>(dst)[in] = q[(row * K + col) / 16];
    if (g == 0 && (b & 1) == 0) {
        const int j = b >> 1;
        const long long grp = row * (K / 128) + 2 * c + j;
        unsigned short *gdst = reinterpret_cast<unsigned short *>(dst + 32768 + 8 * (16 * w + n));
        const unsigned zv = z[grp];
        gdst[j] = s[grp];
        gdst[2 + j] = (unsigned short)(bf16 ? __float_as_uint((float)zv) >> 16 : 0x6400u | zv);
    }
}

struct SkinnyI8 {                                  // the dense INT8 kernel and its DEPTH row, for gemm_skinny_q_call
    static constexpr int depth(int rt) { return rt == 4 ? 3 : 4; }
    template <typename TT, int RT> static constexpr auto kern() { return k_gemm_skinny_i8<TT, RT, depth(RT)>; }
};

extern "C" {

int samd_gemm_pack_i8(const void *d_q, const void *d_z, const void *d_s, void *d_out, int32_t N, int32_t K, int32_t dtype, void *stream) {
    if (!d_q || !d_z || !d_s || !d_out || d_q == d_out || d_z == d_out || d_s == d_out || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC ||
        K % GEMM_KC != 0 || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_pack_i8: needs N %% 128 == 0, K %% 256 == 0, dtype fp16 or bf16 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long units = (long long)N * K / 16;
    hipLaunchKernelGGL(k_gemm_pack_i8, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_q,
                       (const unsigned char *)d_z, (const unsigned short *)d_s, (unsigned char *)d_out, N, K, dtype == SAMD_BF16 ? 1 : 0);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_gemm_skinny_i8(const void *d_A, const void *d_W8p, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial, void *d_out,
                        int32_t dtype, void *stream) {
    return gemm_skinny_q_call<SkinnyI8>("samd_gemm_skinny_i8", d_A, d_W8p, rows_pad, N, K, splits, d_partial, d_out, dtype, stream);
}

}  // extern "C"

// ================================================================================================
// Mixture-of-experts MLP (Qwen3-MoE: HF Qwen3MoeSparseMoeBlock): router, gathered expert gate|up + SiLU, gathered expert down + combine.
// A sparse layer streams a data-dependent subset of E small matrices, each for its own subset of rows; the choice is made on the device
// and every launch has a fixed grid, so a decode step stays one hipGraph replay.
//   samd_moe_route         k_moe_route (one 16-wave workgroup per row, four experts in flight per wave: fp32 router logits, fp32 softmax, top-k by value with ties to the lower
//                          expert, renormalisation, ONE rounding of the weights), then k_moe_lists (one workgroup): the compacted list of
//                          active experts in ascending order and, per active expert, its (row, slot) entries in ascending order -- fixed
//                          orders, no atomics, so the lists do not depend on which workgroup ran first.
//   samd_moe_gate_up_silu  grid (I / 64 column tiles, min(E, rows * k) active slots); workgroups past the active count exit at once.  The
//                          stream is k_gemm_skinny's with EPI 1 (tile = 64 gate | 64 up columns of ONE expert; expert e's packed matrix at
//                          e * 2 I * H elements); the A tile is GATHERED: tile row r is row lists[a][r] / k of h (an indirection on the
//                          LDS-DMA's per-lane source address, no copy); act row lists[a][r] = row * k + slot receives silu(gate) * up.
//   samd_moe_down_combine  the same stream with EPI 0 over the expert's act rows; y[row * k + slot] gets its own row (no atomics), then
//                          k_moe_combine adds a row's k products in slot order in fp32, weighted, and rounds once.
// Row independence: tile row r of a workgroup depends on A row r and the expert's weights only, the k order is the chunk order (no
// split-K), and the combine's order is the slot order -- a row's output has the same bits whatever else shares the launch, whichever
// tile row or row bucket it lands in.
//   ROUTING WORKSPACE (int32 words at the head of d_ws): [0] n_active; [16 + a] expert of active slot a; [272 + a] its entry count;
//   [528 + 64 a + q] its q-th entry p = row * k + slot.  The down products y [rows * k][hidden] (model dtype) follow at MOE_WS_Y_OFF bytes.
// Tile rows past an expert's count read its first entry's row again (their sums are not written); entries are < rows * k by construction.
// (The MOE_WS_* / MOEW_WS_* word offsets sit with the expert side that reads them: THE SIDE, above the 4-bit streaming body.)
// ================================================================================================

// Router logits stay in fp32 (HF's low-precision F.linear rounds them to the model dtype, which manufactures exact ties: a documented
// difference).  Rows >= *d_n get index -1 and weight 0: they route nowhere.
// 16 waves per row; a wave takes FOUR experts at a time (e0 = 4 w, 4 w + 64, ...), so the h unit and four independent weight units of every
// step are in flight together: Qwen3-30B-A3B (E = 128, H = 2048) is two rounds of four steps per wave instead of 32 experts one after another.
// Every expert's sum keeps one order (k ascending per lane, then a fixed shuffle tree), whatever group it falls in.
#define MOE_ROUTE_WAVES 16
template <typename E>
__global__ __launch_bounds__(64 * MOE_ROUTE_WAVES) void k_moe_route(const E *__restrict__ h, const E *__restrict__ Wr, const int *__restrict__ d_n, int hidden, int n_exp, int top_k,
                                                   int norm_topk, int *__restrict__ topk_idx, E *__restrict__ topk_w) {
    __shared__ float logit[MOE_MAX_E];
    const int row = blockIdx.x, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    if (row >= d_n[0]) {
        if (tid < top_k) { topk_idx[row * top_k + tid] = -1; topk_w[row * top_k + tid] = (E)0.f; }
        return;
    }
    const uint4 *hx = reinterpret_cast<const uint4 *>(h + (size_t)row * hidden);
    for (int e0 = 4 * w; e0 < n_exp; e0 += 4 * MOE_ROUTE_WAVES) {    // 16-byte loads, fp32 sums, a fixed reduction tree
        const uint4 *wx[4];
        float s[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const int e = e0 + i < n_exp ? e0 + i : n_exp - 1; wx[i] = reinterpret_cast<const uint4 *>(Wr + (size_t)e * hidden); s[i] = 0.f; }
#pragma unroll 4
        for (int u = l; u < hidden / 8; u += 64) {               // (unrolled: the loads of four steps x four experts are requested together)
            const uint4 a = hx[u];
            uint4 b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) b[i] = wx[i][u];
            const E *ae = reinterpret_cast<const E *>(&a);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const E *be = reinterpret_cast<const E *>(&b[i]);
#pragma unroll
                for (int j = 0; j < 8; j++) s[i] = fmaf((float)ae[j], (float)be[j], s[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
            if (l == 0 && e0 + i < n_exp) logit[e0 + i] = s[i];
        }
    }
    __syncthreads();
    if (w != 0) return;
    constexpr float NINF = -__builtin_huge_valf();
    float v[MOE_MAX_E / 64];
    float mx = NINF;
#pragma unroll
    for (int i = 0; i < MOE_MAX_E / 64; i++) { const int e = l + 64 * i; v[i] = e < n_exp ? logit[e] : NINF; mx = fmaxf(mx, v[i]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < MOE_MAX_E / 64; i++) se += (l + 64 * i < n_exp) ? expf(v[i] - mx) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    float sel_p[MOE_MAX_K];
    int sel_i[MOE_MAX_K];
    float sum_sel = 0.f;
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; j++) {
        sel_p[j] = 0.f; sel_i[j] = -1;
        if (j >= top_k) continue;
        float bv = NINF; int bi = 0x7fffffff;                    // the largest remaining logit; ties go to the lower expert
#pragma unroll
        for (int i = 0; i < MOE_MAX_E / 64; i++) { const int e = l + 64 * i; if (e < n_exp && (v[i] > bv || (v[i] == bv && e < bi && v[i] > NINF))) { bv = v[i]; bi = e; } }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
#pragma unroll
        for (int i = 0; i < MOE_MAX_E / 64; i++) if (bi == l + 64 * i) v[i] = NINF;
        if (bi < n_exp) { sel_i[j] = bi; sel_p[j] = expf(bv - mx) / se; sum_sel += sel_p[j]; }
    }
    if (l == 0) {
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; j++) {
            if (j >= top_k) continue;
            topk_idx[row * top_k + j] = sel_i[j];
            topk_w[row * top_k + j] = (E)(norm_topk ? sel_p[j] / sum_sel : sel_p[j]);
        }
    }
}

// the lists of samd_moe_route from topk_idx [rows][k] (also on its own: samd_moe_lists, for routing that was decided elsewhere).  Entries of
// rows >= *d_n, indices outside [0, n_exp) and anything past 64 entries of one expert are left out.
__global__ __launch_bounds__(MOE_MAX_E) void k_moe_lists(const int *__restrict__ topk_idx, const int *__restrict__ d_n, int rows, int n_exp, int top_k, int *__restrict__ ws) {
    // one bitmap of entries per expert (bit p of expert e: entry p = row * k + slot routes to e), set with LDS bit-or -- whatever order the
    // threads arrive in, the bitmap is the same -- then every expert's thread walks ITS bits in ascending order: work goes by an expert's own
    // count, not by the rows * k entries
    constexpr int WORDS = MOE_MAX_ROWS * MOE_MAX_K / 32;
    __shared__ unsigned bits[MOE_MAX_E][WORDS + 1];              // (+1: the experts' rows fall on different banks)
    __shared__ int wave_active[MOE_MAX_E / 64];
    const int tid = threadIdx.x, total = rows * top_k;
    int n = d_n[0];
    n = n < 0 ? 0 : (n > rows ? rows : n);
#pragma unroll
    for (int i = 0; i < WORDS; i++) bits[tid][i] = 0u;
    __syncthreads();
    for (int p = tid; p < total; p += MOE_MAX_E) {
        const int r = p / top_k;
        int e = r < n ? topk_idx[p] : -1;
        if (e >= n_exp) e = -1;
        for (int q = r * top_k; q < p; q++) if (topk_idx[q] == e) e = -1;        // an expert counts once per row: its first slot
        if (e >= 0) atomicOr(&bits[e][p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    int c = 0;
#pragma unroll
    for (int i = 0; i < WORDS; i++) c += __popc(bits[tid][i]);
    if (c > MOE_MAX_ROWS) c = MOE_MAX_ROWS;                      // (cannot happen with one slot per row and <= 64 rows: a guard for the list's size)
    // this expert's place among the active ones (ascending expert order): the wave's ballot below this lane + the waves before it
    const unsigned long long act = __ballot(c > 0);
    if ((tid & 63) == 0) wave_active[tid >> 6] = __popcll(act);
    __syncthreads();
    int a = __popcll(act & ((1ull << (tid & 63)) - 1ull));
    for (int w = 0; w < (tid >> 6); w++) a += wave_active[w];
    if (c > 0) {
        ws[MOE_WS_ACTIVE + a] = tid;
        ws[MOE_WS_COUNT + a] = c;
        int q = 0;
#pragma unroll
        for (int i = 0; i < WORDS; i++) {
            unsigned m = bits[tid][i];
            while (m && q < MOE_MAX_ROWS) { ws[MOE_WS_LIST + MOE_MAX_ROWS * a + q++] = 32 * i + (__ffs(m) - 1); m &= m - 1u; }
        }
    }
    if (tid == MOE_MAX_E - 1) ws[0] = a + (c > 0);
}

// One expert's share of a projection: k_gemm_skinny's stream (GEMM_KC chunks, 8 waves x 16 columns, hand-issued nt weight loads with counted
// vmcnt, LDS-DMA'd A tiles with the XOR swizzle on the source address, two chunks in flight) behind the expert side (THE SIDE, above the
// 4-bit streaming body), with in-out load destinations (THE PIPELINE, there).
// GU: W = gate|up tiles (64 gate | 64 up columns), A = h, out = act; otherwise W = down tiles, A = act, out = y.
template <typename TT, int RT, bool GU, bool WIDE = false>
__device__ __forceinline__ void moe_expert_gemm(const typename TT::elem *__restrict__ A, const typename TT::elem *__restrict__ W, const int *__restrict__ ws,
                                                typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int top_k) {
    typedef typename TT::elem E;
    typedef typename TT::vec8 V8;
    constexpr int DEPTH = 2;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 8 + XV;                     // memory operations per thread and chunk
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    if (moe_side_idle(ws)) return;
    const MoeSlot slot = moe_side_open<R, WIDE>(ws);
    int srow[XV];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XV; i++) srow[i] = moe_side_row<GU>(i, top_k);

    const char *wtile = reinterpret_cast<const char *>(W) + ((size_t)slot.expert * (N / GEMM_COLS) + blockIdx.x) * n_chunks * 65536;
    const uint32_t wlane = (uint32_t)tid * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    u32x4 wr[DEPTH][4][2];
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
#pragma unroll
        for (int b = 0; b < 4; b++) asm volatile("" : "=v"(wr[d][b][0]), "=v"(wr[d][b][1]));
    auto load_wb = [&](u32x4 (&dst)[4][2], int c, int b) {
        const char *p = wtile + (size_t)c * 65536;
#pragma unroll
        for (int j = 0; j < 2; j++)
            asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "+v"(dst[b][j]) : "v"(wlane), "s"(p + 8192 * (2 * b + j)) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)srow[i] * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4][2], int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    auto phase = [&](u32x4 (&cur)[4][2], int c, int buf) {
        gemm_wait_younger<DEPTH, PC>(n_chunks - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            gemm_read_a2<RT>(r, a0, a1);
            // re-defined behind the counted wait (volatile asm keeps its order): no use can be scheduled above it
            asm volatile("" : "+v"(cur[b][0]), "+v"(cur[b][1]) : : "memory");
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][0]), __builtin_bit_cast(V8, cur[b][0]), acc[mt]);
                acc[mt] = TT::mfma(__builtin_bit_cast(V8, r[mt][1]), __builtin_bit_cast(V8, cur[b][1]), acc[mt]);
            }
            if (RT >= 3 && c + DEPTH < n_chunks) {             // 48 / 64 rows: refill per k block (see k_gemm_skinny)
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
            }
        }
        if (RT < 3 && c + DEPTH < n_chunks) { load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if (d < n_chunks) { load_w(wr[d], d); stage_x(d, d); }
    int buf = 0;
    for (int c = 0; c < n_chunks; c += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c + d < n_chunks) { phase(wr[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
    }
    moe_side_store<TT, RT, GU>(acc, slot.cnt, out, N, reinterpret_cast<float *>(gemm_lds), w, n, g);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT >= 3 ? 2 : GEMM_WAVES / 2) void k_moe_gate_up_silu(const typename TT::elem *__restrict__ h, const typename TT::elem *__restrict__ W,
                                                                                                    const int *__restrict__ ws, typename TT::elem *__restrict__ act,
                                                                                                    int K, int N, int n_chunks, int top_k) {
    moe_expert_gemm<TT, RT, true>(h, W, ws, act, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT >= 3 ? 2 : GEMM_WAVES / 2) void k_moe_down(const typename TT::elem *__restrict__ act, const typename TT::elem *__restrict__ W,
                                                                                            const int *__restrict__ ws, typename TT::elem *__restrict__ y,
                                                                                            int K, int N, int n_chunks, int top_k) {
    moe_expert_gemm<TT, RT, false>(act, W, ws, y, K, N, n_chunks, top_k);
}

// out[row] = sum_j w[row][j] * y[row * k + j], j = 0 .. k - 1 in order, fp32, one rounding; rows >= *d_n and slots without a valid expert (or repeating an earlier slot's) add nothing
template <typename E>
__global__ __launch_bounds__(256) void k_moe_combine(const E *__restrict__ y, const int *__restrict__ topk_idx, const E *__restrict__ topk_w, const int *__restrict__ d_n,
                                                     E *__restrict__ out, int hidden, int top_k, int n_exp) {
    const int row = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x;
    if (u >= hidden / 8) return;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0.f;
    if (row < d_n[0]) {
        for (int j = 0; j < top_k; j++) {
            const int e = topk_idx[row * top_k + j];
            bool skip = e < 0 || e >= n_exp;                     // what k_moe_lists left out has no product: it adds nothing
            for (int q = 0; q < j; q++) skip = skip || topk_idx[row * top_k + q] == e;
            if (skip) continue;
            const float wj = (float)topk_w[row * top_k + j];
            const uint4 v = reinterpret_cast<const uint4 *>(y + (size_t)(row * top_k + j) * hidden)[u];
            const E *ve = reinterpret_cast<const E *>(&v);
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i] += wj * (float)ve[i];
        }
    }
    uint4 o;
    E *oe = reinterpret_cast<E *>(&o);
#pragma unroll
    for (int i = 0; i < 8; i++) oe[i] = (E)acc[i];
    reinterpret_cast<uint4 *>(out + (size_t)row * hidden)[u] = o;
}

// E experts of row-major [N][K] each, end to end -> each in k_gemm_pack's 128-column tile layout, end to end.  half > 0 (gate|up, half = I):
// packed row 128 t + q is gate row 64 t + q for q < 64 and up row 64 t + q - 64 otherwise, so that a tile holds matching columns.
__global__ __launch_bounds__(256) void k_moe_pack(const uint4 *__restrict__ W, uint4 *__restrict__ out, int N, int K, int half, long long total) {
    const long long ug = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ug >= total) return;
    const long long per = (long long)N * K / 8, e = ug / per, u = ug % per;
    const int n_chunks = K / GEMM_KC;
    const long long blk = u >> 12;
    const int in = (int)(u & 4095), jj = in >> 9, tid = in & 511, w = tid >> 6, g = (tid >> 4) & 3, n = tid & 15;
    const int t = (int)(blk / n_chunks), c = (int)(blk % n_chunks), b = jj >> 1, j = jj & 1;
    const int q = 16 * w + n;
    const long long row = half ? (q < 64 ? 64LL * t + q : (long long)half + 64LL * t + q - 64) : 128LL * t + q;
    const long long col = 256LL * c + 64 * b + 16 * g + 8 * j;
    out[ug] = W[e * per + (row * K + col) / 8];
}

template <bool GU>
static hipError_t moe_gemm_dispatch(int dtype, int rows_pad, dim3 grid, hipStream_t st, const void *A, const void *W, const int *ws, void *out, int K, int N, int top_k) {
#define GO(TT, RT) return stream_launch<(GU ? k_moe_gate_up_silu<TT, RT> : k_moe_down<TT, RT>), stream_lds(2, RT)>( \
        grid, st, (const typename TT::elem *)A, (const typename TT::elem *)W, ws, (typename TT::elem *)out, K, N, K / GEMM_KC, top_k)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1); else if (rows_pad == 32) GO(TT, 2); else if (rows_pad == 48) GO(TT, 3); else GO(TT, 4); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
}

static bool moe_shape_ok(int rows_pad, int hidden, int moe_inter, int n_experts, int top_k, int dtype) {
    return (rows_pad == 16 || rows_pad == 32 || rows_pad == 48 || rows_pad == 64) && hidden >= GEMM_KC && hidden % GEMM_KC == 0 &&
           moe_inter >= GEMM_KC && moe_inter % GEMM_KC == 0 && n_experts >= 1 && n_experts <= MOE_MAX_E && top_k >= 1 && top_k <= MOE_MAX_K &&
           top_k <= n_experts && (dtype == SAMD_F16 || dtype == SAMD_BF16);
}
#define MOE_SHAPE_MSG "unsupported shape (rows 16/32/48/64, hidden %% 256 == 0, moe_intermediate %% 256 == 0, experts <= 256, top-k <= 8, f16/bf16) or null pointer"

// the slot dimension of an expert launch's grid: the shape's upper bound of active experts
static inline int moe_slot_bound(int rows_pad, int n_experts, int top_k) { return n_experts < rows_pad * top_k ? n_experts : rows_pad * top_k; }

// k_moe_combine over `rows` rows of the down products y, behind every format's down launch
static void moe_combine_launch(int dtype, hipStream_t st, const void *y, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_out, int rows, int hidden,
                               int top_k, int n_experts) {
    const dim3 cgrid((hidden / 8 + 255) / 256, rows);
    if (dtype == SAMD_F16)
        hipLaunchKernelGGL(k_moe_combine<_Float16>, cgrid, dim3(256), 0, st, (const _Float16 *)y, d_topk_idx, (const _Float16 *)d_topk_w, d_n, (_Float16 *)d_out, hidden, top_k, n_experts);
    else
        hipLaunchKernelGGL(k_moe_combine<__bf16>, cgrid, dim3(256), 0, st, (const __bf16 *)y, d_topk_idx, (const __bf16 *)d_topk_w, d_n, (__bf16 *)d_out, hidden, top_k, n_experts);
}

extern "C" {

int32_t samd_moe_workspace_layout(int32_t field) {
    switch (field) {
    case 0: return MOE_WS_ACTIVE;
    case 1: return MOE_WS_COUNT;
    case 2: return MOE_WS_LIST;
    case 3: return MOE_MAX_ROWS;
    case 4: return MOE_WS_INTS;
    default: return -1;
    }
}

int64_t samd_moe_workspace(int32_t rows_pad, int32_t hidden, int32_t n_experts, int32_t top_k, int32_t dtype) {
    (void)n_experts; (void)dtype;
    return (int64_t)MOE_WS_Y_OFF + (int64_t)rows_pad * top_k * hidden * 2;
}

int samd_moe_pack_experts(const void *d_W, void *d_packed, int32_t n_experts, int32_t N, int32_t K, int32_t gate_up, void *stream) {
    if (!d_W || !d_packed || d_W == d_packed || n_experts < 1 || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0) {
        samd_set_error("samd_moe_pack_experts: needs N %% 128 == 0, K %% 256 == 0 and distinct buffers"); return SAMD_E_INVALID;
    }
    const long long total = (long long)n_experts * N * K / 8;
    hipLaunchKernelGGL(k_moe_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)d_W, (uint4 *)d_packed, N, K,
                       gate_up ? N / 2 : 0, total);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_lists(const int32_t *d_topk_idx, const int32_t *d_n, int32_t rows_pad, int32_t n_experts, int32_t top_k, void *d_ws, void *stream) {
    if (!d_topk_idx || !d_n || !d_ws || !moe_shape_ok(rows_pad, GEMM_KC, GEMM_KC, n_experts, top_k, SAMD_F16)) {
        samd_set_error("samd_moe_lists: " MOE_SHAPE_MSG); return SAMD_E_INVALID;
    }
    hipLaunchKernelGGL(k_moe_lists, dim3(1), dim3(MOE_MAX_E), 0, (hipStream_t)stream, d_topk_idx, d_n, rows_pad, n_experts, top_k, (int *)d_ws);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_route(const void *d_h, const void *d_router, const int32_t *d_n, int32_t rows_pad, int32_t hidden, int32_t n_experts, int32_t top_k, int32_t norm_topk,
                   int32_t *d_topk_idx, void *d_topk_w, void *d_ws, int32_t dtype, void *stream) {
    if (!d_h || !d_router || !d_n || !d_topk_idx || !d_topk_w || !d_ws || !moe_shape_ok(rows_pad, hidden, GEMM_KC, n_experts, top_k, dtype)) {
        samd_set_error("samd_moe_route: " MOE_SHAPE_MSG); return SAMD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SAMD_F16)
        hipLaunchKernelGGL(k_moe_route<_Float16>, dim3(rows_pad), dim3(64 * MOE_ROUTE_WAVES), 0, st, (const _Float16 *)d_h, (const _Float16 *)d_router, d_n, hidden, n_experts, top_k, norm_topk,
                           d_topk_idx, (_Float16 *)d_topk_w);
    else
        hipLaunchKernelGGL(k_moe_route<__bf16>, dim3(rows_pad), dim3(64 * MOE_ROUTE_WAVES), 0, st, (const __bf16 *)d_h, (const __bf16 *)d_router, d_n, hidden, n_experts, top_k, norm_topk,
                           d_topk_idx, (__bf16 *)d_topk_w);
    LAUNCHCHK();
    return samd_moe_lists(d_topk_idx, d_n, rows_pad, n_experts, top_k, d_ws, stream);
}

int samd_moe_gate_up_silu(const void *d_h, const void *d_Wgu, const void *d_ws, int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k,
                          void *d_act, int32_t dtype, void *stream) {
    if (!d_h || !d_Wgu || !d_ws || !d_act || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype)) {
        samd_set_error("samd_moe_gate_up_silu: " MOE_SHAPE_MSG); return SAMD_E_INVALID;
    }
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe_gemm_dispatch<true>(dtype, rows_pad, dim3(2 * moe_inter / GEMM_COLS, bound), (hipStream_t)stream, d_h, d_Wgu, (const int *)d_ws, d_act, hidden,
                                                 2 * moe_inter, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_gate_up_silu: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_down_combine(const void *d_act, const void *d_Wdown, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws, int32_t rows_pad,
                          int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, void *d_out, int32_t dtype, void *stream) {
    if (!d_act || !d_Wdown || !d_topk_idx || !d_topk_w || !d_n || !d_ws || !d_out || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype)) {
        samd_set_error("samd_moe_down_combine: " MOE_SHAPE_MSG); return SAMD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    void *y = (char *)d_ws + MOE_WS_Y_OFF;
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe_gemm_dispatch<false>(dtype, rows_pad, dim3(hidden / GEMM_COLS, bound), st, d_act, d_Wdown, (const int *)d_ws, y, moe_inter, hidden, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_down_combine: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    moe_combine_launch(dtype, st, y, d_topk_idx, d_topk_w, d_n, d_out, rows_pad, hidden, top_k, n_experts);
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"

// ================================================================================================
// Mixture-of-experts MLP with 4-bit experts: gemm_stream_w4, the dense calls' body with their weight policies W4Mx / W4Int, on the expert
// side (THE SIDE, above that body) -- the kernels below are its SIDE_EXPERT instantiations at MoeW4Depth.
//   samd_moe_gate_up_silu_f4 / _i4, samd_moe_down_combine_f4 / _i4: the fixed grid (N / 128, min(E, rows_pad * top_k)), the routing
//   workspace and k_moe_combine are those of the model-dtype calls; the weight side is the dense one: 17 KiB (tile, chunk) blocks, two
//   16-byte nt element loads and one nt side-data load per lane and chunk, the widening behind the counted wait, the A-side unit order
//   (16 j + 4 g + i) ^ n, fp32 accumulation in chunk order.  No split-K, no atomics: a row's output has the same bits whatever shares the
//   launch.
//   PACKED LAYOUT, MXFP4: the experts laid end to end are ONE matrix of E * N rows in samd_gemm_pack_f4's layout; expert e's tile t is global
//   tile e * N / 128 + t, at ((e * N / 128 + t) * K / 256 + c) * 17408 bytes for chunk c.  gate|up: packed row 128 t + r of an expert is its
//   gate row 64 t + r for r < 64 and its up row I + 64 t + r - 64 otherwise (samd_hip/moe.py permutes q and e8 before packing; MX blocks run
//   along k, so whole blocks move), which is the interleave of k_moe_pack: waves 0-3 hold gate columns, waves 4-7 the up columns they meet.
//   PACKED LAYOUT, INT4 (AWQ / GPTQ; W = rne_dtype((q - z) * s), one rounding): the same in samd_gemm_pack_i4's layout (the pack call with
//   N := E * N), the same tile addresses.  gate|up: the rows are permuted before packing as for MXFP4 (samd_hip/moe.py: gate_up_tile_order;
//   groups run along k, so whole rows move with their zero points and scales).  The buffer is dtype-specific (the scales and the pre-biased
//   zero points are in the model dtype).
//   DEPTH (chunks of 16 KiB + 1 KiB in flight per workgroup), one table for both formats, chosen per row tile under (DEPTH - 1) * PC <= 63
//   (vmcnt: 28, 10, 6, 14), (DEPTH + 1) A buffers of R * 512 bytes + the list (256 bytes, 1 KiB of static LDS after alignment) inside 160 KiB
//   of LDS for the intended workgroups per CU, and no spills: 16 rows 8 (9 x 8 KiB = 72 KiB, two workgroups per CU; an expert's whole gate|up
//   stream of hidden 2048 is in flight from the prologue), 32 rows 3 (4 x 16 = 64 KiB, two per CU -- the dense 4 would need 2 x (80 + 1) KiB
//   > 160 KiB with the list), 48 rows 2 (3 x 24 = 72 KiB, two per CU: expert streams are 1-8 chunks long, so a second workgroup that covers
//   the first one's prologue and epilogue is worth more than depth; one per CU would allow 5), 64 rows 3 (4 x 32 = 128 KiB, one per CU: two
//   never fit).  INT4's group data costs one VGPR per chunk in flight more than MXFP4's scales (8 more at 16 rows) and every instantiation
//   still compiles without scratch (tests/test_moe_int4_cpu.py reads it from the code object's metadata).  An expert's stream is often
//   SHORTER than the depth (3 chunks for down at moe_inter 768, 1 at 256): the skipped prologue loads leave their in-out destination
//   registers as they are (THE PIPELINE, at gemm_stream_w4).  Not swept on a GPU; profiles/moe_experts_mxfp4.md and profiles/moe_experts_int4.md have
//   the timings.
// ================================================================================================
template <int RT> struct MoeW4Depth { static constexpr int value = RT == 1 ? 8 : RT == 3 ? 2 : 3; };

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe4_gate_up_silu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W4,
                                                                         const int *__restrict__ ws, typename TT::elem *__restrict__ act,
                                                                         int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Mx, TT, RT, MoeW4Depth<RT>::value, SIDE_EXPERT, true>(h, W4, ws, nullptr, act, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe4_down(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W4,
                                                                 const int *__restrict__ ws, typename TT::elem *__restrict__ y,
                                                                 int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Mx, TT, RT, MoeW4Depth<RT>::value, SIDE_EXPERT, false>(act, W4, ws, nullptr, y, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe_i4_gate_up_silu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W4,
                                                                           const int *__restrict__ ws, typename TT::elem *__restrict__ act,
                                                                           int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Int, TT, RT, MoeW4Depth<RT>::value, SIDE_EXPERT, true>(h, W4, ws, nullptr, act, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe_i4_down(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W4,
                                                                   const int *__restrict__ ws, typename TT::elem *__restrict__ y,
                                                                   int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Int, TT, RT, MoeW4Depth<RT>::value, SIDE_EXPERT, false>(act, W4, ws, nullptr, y, K, N, n_chunks, top_k);
}

// the 4-bit expert kernels and their DEPTH table, for the host-side templates below (MoeI8 is the INT8 one)
template <typename F> struct MoeW4 {
    template <int RT> static constexpr int depth = MoeW4Depth<RT>::value;
    template <typename TT, int RT, bool GU> static constexpr auto kern() {
        return F::mx ? (GU ? k_moe4_gate_up_silu<TT, RT> : k_moe4_down<TT, RT>) : (GU ? k_moe_i4_gate_up_silu<TT, RT> : k_moe_i4_down<TT, RT>);
    }
};

// X: a quantised expert format whose kernels take (A, packed W, ws, out, K, N, chunks, top_k) -- MoeW4<W4Mx>, MoeW4<W4Int>, MoeI8.  The
// model-dtype and block-scaled FP8 calls stay apart: the first casts W to the model dtype, the second adds a scale table, a bound on K
// and a message of its own.
template <typename X, bool GU>
static hipError_t moe_q_gemm_dispatch(int dtype, int rows_pad, dim3 grid, hipStream_t st, const void *A, const void *W, const int *ws, void *out, int K, int N, int top_k) {
#define GO(TT, RT) return stream_launch<X::template kern<TT, RT, GU>(), stream_lds(X::template depth<RT>, RT)>( \
        grid, st, (const typename TT::elem *)A, (const unsigned char *)W, ws, (typename TT::elem *)out, K, N, K / GEMM_KC, top_k)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1); else if (rows_pad == 32) GO(TT, 2); else if (rows_pad == 48) GO(TT, 3); else GO(TT, 4); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
}

template <typename X>
static int moe_q_gate_up_silu(const char *fn, const void *d_h, const void *d_Wgu, const void *d_ws, int rows_pad, int hidden, int moe_inter, int n_experts, int top_k,
                              void *d_act, int dtype, void *stream) {
    if (!d_h || !d_Wgu || !d_ws || !d_act || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype)) {
        samd_set_error("%s: " MOE_SHAPE_MSG, fn); return SAMD_E_INVALID;
    }
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe_q_gemm_dispatch<X, true>(dtype, rows_pad, dim3(2 * moe_inter / GEMM_COLS, bound), (hipStream_t)stream, d_h, d_Wgu, (const int *)d_ws, d_act,
                                                      hidden, 2 * moe_inter, top_k);
    if (e != hipSuccess) { samd_set_error("%s: %s", fn, hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

template <typename X>
static int moe_q_down_combine(const char *fn, const void *d_act, const void *d_Wdown, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws,
                              int rows_pad, int hidden, int moe_inter, int n_experts, int top_k, void *d_out, int dtype, void *stream) {
    if (!d_act || !d_Wdown || !d_topk_idx || !d_topk_w || !d_n || !d_ws || !d_out || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype)) {
        samd_set_error("%s: " MOE_SHAPE_MSG, fn); return SAMD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    void *y = (char *)d_ws + MOE_WS_Y_OFF;
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe_q_gemm_dispatch<X, false>(dtype, rows_pad, dim3(hidden / GEMM_COLS, bound), st, d_act, d_Wdown, (const int *)d_ws, y, moe_inter, hidden, top_k);
    if (e != hipSuccess) { samd_set_error("%s: %s", fn, hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    moe_combine_launch(dtype, st, y, d_topk_idx, d_topk_w, d_n, d_out, rows_pad, hidden, top_k, n_experts);
    LAUNCHCHK();
    return SAMD_OK;
}

extern "C" {

int samd_moe_gate_up_silu_f4(const void *d_h, const void *d_Wgu4, const void *d_ws, int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts,
                             int32_t top_k, void *d_act, int32_t dtype, void *stream) {
    return moe_q_gate_up_silu<MoeW4<W4Mx>>("samd_moe_gate_up_silu_f4", d_h, d_Wgu4, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_act, dtype, stream);
}

int samd_moe_down_combine_f4(const void *d_act, const void *d_Wdown4, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws,
                             int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, void *d_out, int32_t dtype, void *stream) {
    return moe_q_down_combine<MoeW4<W4Mx>>("samd_moe_down_combine_f4", d_act, d_Wdown4, d_topk_idx, d_topk_w, d_n, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_out, dtype,
                                     stream);
}

int samd_moe_gate_up_silu_i4(const void *d_h, const void *d_Wgu4, const void *d_ws, int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts,
                             int32_t top_k, void *d_act, int32_t dtype, void *stream) {
    return moe_q_gate_up_silu<MoeW4<W4Int>>("samd_moe_gate_up_silu_i4", d_h, d_Wgu4, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_act, dtype, stream);
}

int samd_moe_down_combine_i4(const void *d_act, const void *d_Wdown4, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws,
                             int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, void *d_out, int32_t dtype, void *stream) {
    return moe_q_down_combine<MoeW4<W4Int>>("samd_moe_down_combine_i4", d_act, d_Wdown4, d_topk_idx, d_topk_w, d_n, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_out, dtype,
                                      stream);
}

}  // extern "C"

// ================================================================================================
// Mixture-of-experts MLP with INT8 experts (GPTQ: unsigned 8-bit codes, one scale and one 8-bit zero point per 128 elements along k):
// gemm_stream_i8, k_gemm_skinny_i8's body, on the expert side (THE SIDE, above the 4-bit streaming body) -- the kernels below are its
// SIDE_EXPERT / SIDE_WIDE instantiations at MoeI8Depth.
//   samd_moe_gate_up_silu_i8 / samd_moe_down_combine_i8: the fixed grid (N / 128, min(E, rows_pad * top_k)), the routing workspace and
//   k_moe_combine are those of the model-dtype calls, through the host templates of the 4-bit calls.  The weight side is the dense one:
//   33 KiB (tile, chunk) blocks, four 16-byte nt code loads and one 8-byte nt group-data load per lane and chunk with in-out destinations,
//   I8Widen behind the counted wait (W = rne_dtype((q - z) * s), ONE rounding), the A-side unit order (8 b + 2 g) ^ n, fp32 accumulation in
//   chunk order.  No split-K, no atomics: a row's output has the same bits whatever shares the launch.
//   What the 4-bit and the 8-bit kernels share is the side, and that is written once; the phase stays with the format (gemm_stream_i8 says
//   how the two differ), so there are two stream bodies and no 4-bit / 8-bit policy.
//   PACKED LAYOUT: the experts laid end to end are ONE matrix of E * N rows in samd_gemm_pack_i8's layout (the pack call with N := E * N);
//   expert e's tile t is global tile e * N / 128 + t, at ((e * N / 128 + t) * K / 256 + c) * 33792 bytes for chunk c.  gate|up: the rows are
//   permuted before packing as for INT4 (samd_hip/moe.py: gate_up_tile_order; groups run along k, so whole rows move with their zero points
//   and scales).  E * N * K * 33 / 32 bytes; dtype-specific (the scales and the pre-biased zero points are in the model dtype).
//   DEPTH (chunks of 32 KiB + 1 KiB in flight per workgroup), per row tile under (DEPTH - 1) * PC <= 63 with PC = 5 + RT (vmcnt: 18, 14, 8,
//   0), (DEPTH + 1) A buffers of R * 512 bytes + the list (1 KiB of static LDS after alignment) inside 160 KiB for TWO workgroups per CU at
//   every row tile, and 18 VGPRs per chunk in flight inside the 128 registers two workgroups per CU leave a wave, without scratch: 16 rows
//   4 (5 x 8 = 40 KiB; 8 as for 4-bit would need 144 VGPRs), 32 rows 3 (4 x 16 = 64 KiB -- the dense 4 would need 2 x (80 + 1) KiB >
//   160 KiB), 48 rows 2 (3 x 24 = 72 KiB, the 4-bit table's reasoning: expert streams are 1-8 chunks long, so a second workgroup that
//   covers the first one's prologue and epilogue is worth more than depth), 64 rows 1 (2 x 32 = 64 KiB: the per-k-block refill keeps the
//   next chunk's loads in flight behind the block in use, and the second workgroup does the rest).  The 64-row entry was compared on an
//   MI355X against 3 at one workgroup per CU (4 x 32 = 128 KiB, 146 VGPRs), the 4-bit and FP8 tables' choice: 170 against 207 us (bf16)
//   and 164 against 189 us (fp16) for the three-call layer at A3B geometry (profiles/moe_experts_int8.md); the other entries were not
//   swept.  An expert's stream is often SHORTER than the depth (3 chunks for down at moe_inter 768, 1 at 256): the skipped prologue loads
//   leave their in-out destination registers as they are (THE PIPELINE, at gemm_stream_w4).
//   The one-pass-prefill forms are the WIDE instantiations at the 64-row tile (k_moew_i8_gu / k_moew_i8_dn, expert_format code 5: 4 stays
//   unassigned, callers pin it as an unknown code).
// ================================================================================================
template <int RT> struct MoeI8Depth { static constexpr int value = RT == 1 ? 4 : RT == 3 ? 2 : RT == 4 ? 1 : 3; };

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe_i8_gate_up_silu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W8,
                                                                           const int *__restrict__ ws, typename TT::elem *__restrict__ act,
                                                                           int K, int N, int n_chunks, int top_k) {
    gemm_stream_i8<TT, RT, MoeI8Depth<RT>::value, SIDE_EXPERT, true>(h, W8, ws, nullptr, act, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moe_i8_down(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W8,
                                                                   const int *__restrict__ ws, typename TT::elem *__restrict__ y,
                                                                   int K, int N, int n_chunks, int top_k) {
    gemm_stream_i8<TT, RT, MoeI8Depth<RT>::value, SIDE_EXPERT, false>(act, W8, ws, nullptr, y, K, N, n_chunks, top_k);
}

// the one-pass-prefill forms (samd_moe_wide_*, expert_format 5): the 64-row tile over the wide workspace's tile records
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moew_i8_gu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W8, const int *__restrict__ ws,
                                                                  typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    gemm_stream_i8<TT, 4, MoeI8Depth<4>::value, SIDE_WIDE, true>(h, W8, ws, nullptr, act, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_moew_i8_dn(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W8, const int *__restrict__ ws,
                                                                  typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    gemm_stream_i8<TT, 4, MoeI8Depth<4>::value, SIDE_WIDE, false>(act, W8, ws, nullptr, y, K, N, n_chunks, top_k);
}

struct MoeI8 {                                     // the INT8 expert kernels and their DEPTH table, for moe_q_gate_up_silu / moe_q_down_combine
    template <int RT> static constexpr int depth = MoeI8Depth<RT>::value;
    template <typename TT, int RT, bool GU> static constexpr auto kern() { return GU ? k_moe_i8_gate_up_silu<TT, RT> : k_moe_i8_down<TT, RT>; }
};

extern "C" {

int samd_moe_gate_up_silu_i8(const void *d_h, const void *d_Wgu8, const void *d_ws, int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts,
                             int32_t top_k, void *d_act, int32_t dtype, void *stream) {
    return moe_q_gate_up_silu<MoeI8>("samd_moe_gate_up_silu_i8", d_h, d_Wgu8, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_act, dtype, stream);
}

int samd_moe_down_combine_i8(const void *d_act, const void *d_Wdown8, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws,
                             int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, void *d_out, int32_t dtype, void *stream) {
    return moe_q_down_combine<MoeI8>("samd_moe_down_combine_i8", d_act, d_Wdown8, d_topk_idx, d_topk_w, d_n, d_ws, rows_pad, hidden, moe_inter, n_experts, top_k, d_out, dtype,
                                     stream);
}

}  // extern "C"

// ================================================================================================
// Mixture-of-experts MLP with block-scaled FP8 experts (OCP e4m3fn codes, one fp32 scale per 128 x 128 block: the official Qwen3-MoE FP8
// checkpoints' weight / weight_scale_inv): the gathered expert GEMMs of moe_expert_gemm over k_gemm_skinny_f8's 8-bit weight stream.
//   NUMERIC CONTRACT (samd_hip/fp8.py): W[n][k] = float(q[n][k]) * s[n / 128][k / 128], s fp32, finite, positive.  W is never formed:
//   out = sum_b s_b * (sum_{k in block b} A[m][k] * q[n][k]) -- the inner sum an fp32 MFMA accumulation over the block's 128 k with q widened
//   exactly (F8Widen, scale 1), the outer step ONE fp32 FMA per accumulator and block (acc = fma(acc_blk, s_b, acc)), blocks in ascending
//   order: 4 * RT FMAs per lane and block.  Nothing can overflow the model dtype on the way; the epilogues' roundings are unchanged.
//   samd_moe_gate_up_silu_f8 / samd_moe_down_combine_f8: the fixed grid (N / 128, min(E, rows_pad * top_k)) and k_moe_combine are the
//   model-dtype calls'; the expert side is the shared one (THE SIDE, above the 4-bit streaming body), with the scale staging under the
//   list's barrier; the counted waits have in-out load destinations (THE PIPELINE, there); the weight side is k_gemm_skinny_f8's: 32 KiB
//   per (128-column tile, 256-k chunk), four hand-issued nt 16-byte loads per thread and chunk.  No split-K, no atomics: a row's output
//   has the same bits whatever shares the launch.  The weight pipeline is a function of its own (the per-block FMA sits inside the phase).
//   PACKED BUFFER (samd_hip/moe.py: pack_experts_fp8), one per fused tensor: the codes of the E experts laid end to end as ONE matrix of
//   E * N rows in samd_gemm_pack_f8's layout (expert e's tile t is global tile T = e * N / 128 + t, chunk c at (T * K / 256 + c) * 32768
//   bytes; gate|up rows permuted before packing by gate_up_tile_order), then, at the next multiple of 256 bytes, an fp32 table
//   [E * N / 64][K / 128]: one scale per (64 packed rows, 128 k), so that a wave's 16 columns share one scale per k block -- waves 0-3 of
//   tile T read row 2 T, waves 4-7 row 2 T + 1 (gate|up: gate rows 64 t.. = scale row-block t / 2, up rows I + 64 t.. = row-block
//   (I + 64 t) / 128; down: both halves repeat the tile's one scale).
//   THE SCALES never are a dependent global load inside a phase: the tile's 2 * K / 128 scales are staged ONCE into static LDS beside
//   the list, before the stream starts; a phase reads its two (chunk c = k blocks 2 c, 2 c + 1) as one wave-uniform 8-byte LDS read.
//   DEPTH per row tile, as k_gemm_skinny_f8 chose it: 4 chunks of 32 KiB in flight = the model-dtype expert kernel's 128 KiB per workgroup
//   (2 x 64 KiB) and its 64 weight VGPRs, where the 160 KiB of LDS allows DEPTH + 1 A buffers of R * 512 bytes: 16 rows 40 KiB, 32 rows
//   80 KiB, 48 rows 120 KiB; at 64 rows 5 buffers would be the whole 160 KiB, so that tile keeps 3 chunks in flight (4 buffers, 128 KiB,
//   48 weight VGPRs).  Static LDS: the list (256 bytes) + the scales (1 KiB: K <= 16384), 2 KiB as laid out.  With it only the 16-row
//   tile fits two workgroups per CU, and the launch bounds say so: 2 there (128 VGPRs allowed, 112 used: 64 weight + 2 x 4 accumulators +
//   8 A + 8 widened + addresses) and 1 for the others (136 / 158 / 166 VGPRs at 32 / 48 / 64 rows; at 64: 48 weight + 2 x 16
//   accumulators + 32 A + 8 widened).  No instantiation has scratch (tests/test_moe_fp8_cpu.py).  (DEPTH - 1) * PC <= 63: 15, 18, 21, 16.
//   An expert's stream is often SHORTER than the depth; the skipped prologue loads leave their in-out destinations as they are.
//   The table is not swept on a GPU; profiles/moe_experts_fp8.md says what was measured.
// ================================================================================================
#define MOE8_MAX_KB 128                // k blocks of 128 per row: K <= 16384
template <int RT> struct Moe8Depth { static constexpr int value = RT == 4 ? 3 : 4; };

template <typename TT, int RT, bool GU, bool WIDE = false>          // WIDE: a tile record of the wide workspace names the expert and its list
__device__ __forceinline__ void moe8_expert_gemm(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W8, const float *__restrict__ stab,
                                                 const int *__restrict__ ws, typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int top_k) {
    typedef typename TT::elem E;
    constexpr int DEPTH = Moe8Depth<RT>::value;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 4 + XV;                     // memory operations per thread and chunk: 4 weight loads + the A staging
    constexpr size_t WCH = 32768, WU = 8192;       // bytes of one (tile, chunk) block; of one b row inside it
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);
    __shared__ __attribute__((aligned(8))) float scl[2][MOE8_MAX_KB];

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    if (moe_side_idle(ws)) return;
    const MoeSlot slot = moe_side_open<R, WIDE>(ws);
    int srow[XV];
    const size_t tile = (size_t)slot.expert * (N / GEMM_COLS) + blockIdx.x;
    // the tile's scales, under the list's barrier: rows 2 tile (waves 0-3) and 2 tile + 1 (waves 4-7) of the table are contiguous, 2 * K / 128 floats
    if (tid < 4 * n_chunks) scl[tid >= 2 * n_chunks][tid >= 2 * n_chunks ? tid - 2 * n_chunks : tid] = stab[tile * 4 * n_chunks + tid];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < XV; i++) srow[i] = moe_side_row<GU>(i, top_k);

    const char *wtile = reinterpret_cast<const char *>(W8) + tile * n_chunks * WCH;
    const uint32_t wlane = (uint32_t)tid * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];
    const float *sw = scl[w >> 2];                 // this wave's scales, one per k block

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    // the load destinations: one value each, defined once; every load is an in-out operand of it (THE PIPELINE, at gemm_stream_w4)
    u32x4 wr[DEPTH][4];
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
#pragma unroll
        for (int b = 0; b < 4; b++) asm volatile("" : "=v"(wr[d][b]));
    auto load_wb = [&](u32x4 (&dst)[4], int c, int b) {
        const char *p = wtile + (size_t)c * WCH;
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "+v"(dst[b]) : "v"(wlane), "s"(p + WU * b) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)srow[i] * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4], int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    auto phase = [&](u32x4 (&cur)[4], int c, int buf) {
        gemm_wait_younger<DEPTH, PC>(n_chunks - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
        const float2 s2 = *reinterpret_cast<const float2 *>(sw + 2 * c);      // k blocks 2 c and 2 c + 1: an LDS read, ahead of their use
        floatx4 blk[RT];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if ((b & 1) == 0) {
#pragma unroll
                for (int mt = 0; mt < RT; mt++) blk[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
            }
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            gemm_read_a2<RT>(r, a0, a1);
            // re-defined behind the counted wait (volatile asm keeps its order): no conversion can be scheduled above it
            asm volatile("" : "+v"(cur[b]) : : "memory");
            const auto lo = F8Widen<TT>::cvt(cur[b][0], cur[b][1]), hi = F8Widen<TT>::cvt(cur[b][2], cur[b][3]);
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                blk[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][0]), lo, blk[mt]);
                blk[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][1]), hi, blk[mt]);
            }
            if (b & 1) {                                       // a 128-k block is complete: one fp32 FMA per accumulator
                const float s = b == 1 ? s2.x : s2.y;
#pragma unroll
                for (int mt = 0; mt < RT; mt++)
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[mt][q] = __builtin_fmaf(blk[mt][q], s, acc[mt][q]);
            }
            if (RT >= 3 && c + DEPTH < n_chunks) {             // 48 / 64 rows: refill per k block (see k_gemm_skinny)
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
            }
        }
        if (RT < 3 && c + DEPTH < n_chunks) { load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
        if (d < n_chunks) { load_w(wr[d], d); stage_x(d, d); }
    int buf = 0;
    for (int c = 0; c < n_chunks; c += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c + d < n_chunks) { phase(wr[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
    }
    // the block scales went in with the FMAs: the sums are final
    moe_side_store<TT, RT, GU>(acc, slot.cnt, out, N, reinterpret_cast<float *>(gemm_lds), w, n, g);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT == 1 ? 2 : 1) void k_moe8_gate_up_silu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W8,
                                                                                      const float *__restrict__ stab, const int *__restrict__ ws,
                                                                                      typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    moe8_expert_gemm<TT, RT, true>(h, W8, stab, ws, act, K, N, n_chunks, top_k);
}

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT == 1 ? 2 : 1) void k_moe8_down(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W8,
                                                                              const float *__restrict__ stab, const int *__restrict__ ws,
                                                                              typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    moe8_expert_gemm<TT, RT, false>(act, W8, stab, ws, y, K, N, n_chunks, top_k);
}

// the scale table's byte offset inside a packed buffer of `rows` = E * N rows: after the codes, at a multiple of 256 (samd_hip/fp8.py:
// block_scale_offset is the same formula)
static inline size_t moe8_scale_offset(size_t rows, size_t K) { return (rows * K + 255) / 256 * 256; }

template <bool GU>
static hipError_t moe8_gemm_dispatch(int dtype, int rows_pad, dim3 grid, hipStream_t st, const void *A, const void *W8, size_t rows, const int *ws, void *out, int K, int N, int top_k) {
    const float *stab = reinterpret_cast<const float *>(reinterpret_cast<const char *>(W8) + moe8_scale_offset(rows, (size_t)K));
#define GO(TT, RT) return stream_launch<(GU ? k_moe8_gate_up_silu<TT, RT> : k_moe8_down<TT, RT>), stream_lds(Moe8Depth<RT>::value, RT)>( \
        grid, st, (const typename TT::elem *)A, (const unsigned char *)W8, stab, ws, (typename TT::elem *)out, K, N, K / GEMM_KC, top_k)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1); else if (rows_pad == 32) GO(TT, 2); else if (rows_pad == 48) GO(TT, 3); else GO(TT, 4); } while (0)
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
}

#define MOE8_SHAPE_MSG "unsupported shape (rows 16/32/48/64, hidden %% 256 == 0, moe_intermediate %% 256 == 0, both <= 16384, experts <= 256, top-k <= 8, f16/bf16) or null pointer"

extern "C" {

int samd_moe_gate_up_silu_f8(const void *d_h, const void *d_Wgu8, const void *d_ws, int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts,
                             int32_t top_k, void *d_act, int32_t dtype, void *stream) {
    if (!d_h || !d_Wgu8 || !d_ws || !d_act || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype) || hidden > 128 * MOE8_MAX_KB ||
        moe_inter > 128 * MOE8_MAX_KB) {
        samd_set_error("samd_moe_gate_up_silu_f8: " MOE8_SHAPE_MSG); return SAMD_E_INVALID;
    }
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe8_gemm_dispatch<true>(dtype, rows_pad, dim3(2 * moe_inter / GEMM_COLS, bound), (hipStream_t)stream, d_h, d_Wgu8,
                                                  (size_t)n_experts * 2 * moe_inter, (const int *)d_ws, d_act, hidden, 2 * moe_inter, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_gate_up_silu_f8: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_down_combine_f8(const void *d_act, const void *d_Wdown8, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws,
                             int32_t rows_pad, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, void *d_out, int32_t dtype, void *stream) {
    if (!d_act || !d_Wdown8 || !d_topk_idx || !d_topk_w || !d_n || !d_ws || !d_out || !moe_shape_ok(rows_pad, hidden, moe_inter, n_experts, top_k, dtype) ||
        hidden > 128 * MOE8_MAX_KB || moe_inter > 128 * MOE8_MAX_KB) {
        samd_set_error("samd_moe_down_combine_f8: " MOE8_SHAPE_MSG); return SAMD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    void *y = (char *)d_ws + MOE_WS_Y_OFF;
    const int bound = moe_slot_bound(rows_pad, n_experts, top_k);
    const hipError_t e = moe8_gemm_dispatch<false>(dtype, rows_pad, dim3(hidden / GEMM_COLS, bound), st, d_act, d_Wdown8, (size_t)n_experts * hidden,
                                                   (const int *)d_ws, y, moe_inter, hidden, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_down_combine_f8: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    moe_combine_launch(dtype, st, y, d_topk_idx, d_topk_w, d_n, d_out, rows_pad, hidden, top_k, n_experts);
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"

// ================================================================================================
// Dense block-scaled FP8 projection (OCP e4m3fn codes, one fp32 scale per 128 x 128 block: the weight / weight_scale_inv of transformers'
// fine-grained FP8 checkpoints, e.g. Qwen3-*-FP8): out[m][n] = sum_b s[n / 128][b] * (sum_{k in block b} A[m][k] * q[n][k]).
//   NUMERIC CONTRACT (samd_hip/fp8.py), the one of moe8_expert_gemm: the inner sum is an fp32 MFMA accumulation over the block's 128 k with q
//   widened exactly (F8Widen, scale 1); the outer step is ONE fp32 FMA per accumulator and block (acc = fma(blk, s_b, acc)), blocks in
//   ascending order.  W is never formed.  splits == 1: one rounding of the fp32 sum to the model dtype; otherwise fp32 partials
//   [splits][rows_pad][N], as samd_gemm_skinny_f8 writes them.
//   The dense sibling of moe8_expert_gemm with k_gemm_skinny_f8's grid (N / 128, splits), split-K ranges, A staging, k permutation, packed
//   layout (samd_gemm_pack_f8, reused unchanged), hand-issued nt 16-byte weight loads with in-out destinations and counted waits.  A function
//   of its own: every other kernel is left textually alone.
//   THE SCALES are the checkpoint's own table, fp32 [N / 128][K / 128] row-major, not repacked: tile t = block row t, chunk c = entries 2 c
//   and 2 c + 1, so a split reads the contiguous entries [2 c0, 2 c1) of one row.  They arrive as a WAVE-UNIFORM SCALAR LOAD of 8 bytes per
//   chunk (the address depends on blockIdx and the chunk counter only; the pointer is read through the constant address space so that the
//   load is selected as a scalar-memory load whatever the memory clobbers of the hand-written stream say).  Why not staged in LDS as the
//   expert kernel does: (1) a scalar load counts on lgkmcnt, so the counted vmcnt waits (PC = 4 + XV operations per chunk) stay true -- a
//   vector global load inside the stream would break them, and tests/test_fp8b128_cpu.py reads off the code object that there is none;
//   (2) the 32-row tile takes 80 KiB of dynamic LDS and two workgroups fill the CU's 160 KiB exactly: any static LDS would cost it its
//   second workgroup; (3) no table, so no limit on K (Qwen3-32B's down projection has 200 k blocks, more than MOE8_MAX_KB): every
//   K % 256 == 0 that fits int32 is accepted.  The pair of chunk c + 1 is requested during phase c (behind its last A read) and lands in
//   SGPRs while that phase's MFMAs run; the FMAs take the scale as a scalar operand, so the scales cost no VGPR.  The last chunk of a split
//   requests nothing: no read past the table.
//   DEPTH AND LAUNCH BOUNDS per row tile, from the LDS each tile takes and the VGPR counts of the code object (the second launch-bound
//   argument is waves per SIMD: a 512-thread workgroup is 2 waves per SIMD, so two workgroups per CU = 4 waves = 128 VGPRs each).
//   k_gemm_skinny_f8's depths (4 / 4 / 4 / 3) are the starting point; the block accumulators add 4 * RT VGPRs:
//     16 rows: DEPTH 4, 40 KiB LDS, 108 VGPRs -> bound 4, two workgroups per CU as before.
//     32 rows: at DEPTH 4 the code object takes 130 VGPRs unbounded (3 waves per SIMD: ONE workgroup per CU) and spills 3 registers when
//              bounded to 128 -- a spilled load destination would be stored before its data has landed.  DEPTH 3 (48 weight VGPRs, 4 A
//              buffers = 64 KiB) takes 114 VGPRs under bound 4 without spills: two workgroups per CU with 2 x 96 KiB of weights in
//              flight, more than one workgroup's 128 KiB at DEPTH 4.
//     48 rows: DEPTH 4, 120 KiB LDS -> one workgroup per CU whatever the registers; 152 VGPRs, bound 2 (the workgroup's own 2 waves per SIMD).
//     64 rows: DEPTH 3 (5 A buffers would take the whole 160 KiB), 128 KiB LDS, 160 VGPRs, bound 2.
//   (DEPTH - 1) * PC = 15, 12, 21, 16 <= 63.  No instantiation has scratch or VGPR spills, and the only vector global loads are the 16-byte
//   weight loads and the LDS-DMA A loads (tests/test_fp8b128_cpu.py reads both off the code object).  The table is derived from the code
//   object, not swept on a GPU; profiles/fp8b128_gemm.md says what was measured.
// ================================================================================================
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(4))) const f32x2 *cscale2_t;
template <int RT> struct F8bDepth { static constexpr int value = (RT == 2 || RT == 4) ? 3 : 4; };

template <typename TT, int RT>
__global__ __launch_bounds__(64 * GEMM_WAVES, RT <= 2 ? 4 : 2) void k_gemm_skinny_f8b(const typename TT::elem *__restrict__ A, const unsigned char *__restrict__ W8,
                                                                                     const float *__restrict__ sinv, float *__restrict__ partial,
                                                                                     typename TT::elem *__restrict__ out, int K, int N, int n_chunks, int n_splits) {
    typedef typename TT::elem E;
    constexpr int DEPTH = F8bDepth<RT>::value;
    constexpr int R = 16 * RT;
    constexpr int NT = 64 * GEMM_WAVES;
    constexpr int XV = (R * 32) / NT;              // 16-byte units per thread to stage one A chunk (as k_gemm_skinny)
    constexpr int NB = DEPTH + 1;
    constexpr int PC = 4 + XV;                     // memory operations per thread and chunk: 4 weight loads + the A staging
    constexpr size_t WCH = 32768, WU = 8192;       // bytes of one (tile, chunk) block; of one b row inside it
    extern __shared__ __attribute__((aligned(1024))) char gemm_lds[];
    E (*xs)[R][GEMM_KC] = reinterpret_cast<E (*)[R][GEMM_KC]>(gemm_lds);

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    const int n0 = blockIdx.x * GEMM_COLS + 16 * w;
    const int split = blockIdx.y;
    const int c0 = (int)((long long)split * n_chunks / n_splits), c1 = (int)((long long)(split + 1) * n_chunks / n_splits);
    const char *wtile = reinterpret_cast<const char *>(W8) + (size_t)blockIdx.x * n_chunks * WCH;
    const uint32_t wlane = (uint32_t)tid * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lptr_t)&xs[0][0][0];
    // this tile's row of the scale table, two entries per chunk; wave-uniform, read by scalar loads only
    const cscale2_t srow = (cscale2_t)(uintptr_t)(sinv + (size_t)blockIdx.x * 2 * n_chunks);

    floatx4 acc[RT];
#pragma unroll
    for (int mt = 0; mt < RT; mt++) acc[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    // the load destinations: one value each, defined once; every load is an in-out operand of it (THE PIPELINE, at gemm_stream_w4)
    u32x4 wr[DEPTH][4];
#pragma unroll
    for (int d = 0; d < DEPTH; d++)
#pragma unroll
        for (int b = 0; b < 4; b++) asm volatile("" : "=v"(wr[d][b]));
    auto load_wb = [&](u32x4 (&dst)[4], int c, int b) {
        const char *p = wtile + (size_t)c * WCH;
        asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "+v"(dst[b]) : "v"(wlane), "s"(p + WU * b) : "memory");
    };
    auto stage_xi = [&](int c, int buf, int i) {
        const int slot = tid + NT * i, row = slot >> 5, pos = slot & 31, unit = pos ^ (row & 15);
        const E *src = A + (size_t)row * K + (size_t)c * GEMM_KC + 8 * unit;
        E *dst = &xs[buf][0][0] + (size_t)(NT * i + 64 * w) * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        asm volatile("" ::: "memory");
    };
    auto load_w = [&](u32x4 (&dst)[4], int c) {
#pragma unroll
        for (int b = 0; b < 4; b++) load_wb(dst, c, b);
    };
    auto stage_x = [&](int c, int buf) {
#pragma unroll
        for (int i = 0; i < XV; i++) stage_xi(c, buf, i);
    };
    f32x2 snext = (f32x2){0.f, 0.f};               // the scales of the next phase's two k blocks (SGPRs)
    auto phase = [&](u32x4 (&cur)[4], int c, int buf) {
        gemm_wait_younger<DEPTH, PC>(c1 - 1 - c);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const uint32_t xbase = lds_base + (uint32_t)buf * (R * GEMM_KC * 2) + (uint32_t)n * (GEMM_KC * 2);
        const f32x2 s2 = snext;                                // k blocks 2 c and 2 c + 1, requested one phase ago
        floatx4 blk[RT];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if ((b & 1) == 0) {
#pragma unroll
                for (int mt = 0; mt < RT; mt++) blk[mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
            }
            const uint32_t a0 = xbase + (uint32_t)((8 * b + 2 * g) ^ n) * 16, a1 = xbase + (uint32_t)((8 * b + 2 * g + 1) ^ n) * 16;
            u32x4 r[RT][2];
            gemm_read_a2<RT>(r, a0, a1);
            // re-defined behind the counted wait (volatile asm keeps its order): no conversion can be scheduled above it
            asm volatile("" : "+v"(cur[b]) : : "memory");
            if (b == 3 && c + 1 < c1) snext = srow[c + 1];     // behind this phase's last A read (whose wait would otherwise cover it)
            const auto lo = F8Widen<TT>::cvt(cur[b][0], cur[b][1]), hi = F8Widen<TT>::cvt(cur[b][2], cur[b][3]);
#pragma unroll
            for (int mt = 0; mt < RT; mt++) {
                blk[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][0]), lo, blk[mt]);
                blk[mt] = TT::mfma(__builtin_bit_cast(typename TT::vec8, r[mt][1]), hi, blk[mt]);
            }
            if (b & 1) {                                       // a 128-k block is complete: one fp32 FMA per accumulator
                const float s = b == 1 ? s2.x : s2.y;
#pragma unroll
                for (int mt = 0; mt < RT; mt++)
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[mt][q] = __builtin_fmaf(blk[mt][q], s, acc[mt][q]);
            }
            if (RT >= 3 && c + DEPTH < c1) {                   // 48 / 64 rows: refill per k block (see k_gemm_skinny)
                load_wb(cur, c + DEPTH, b);
                if (b < XV) stage_xi(c + DEPTH, buf == 0 ? NB - 1 : buf - 1, b);
            }
        }
        if (RT < 3 && c + DEPTH < c1) { load_w(cur, c + DEPTH); stage_x(c + DEPTH, buf == 0 ? NB - 1 : buf - 1); }
    };
    if (c0 < c1) {
        snext = srow[c0];
#pragma unroll
        for (int d = 0; d < DEPTH; d++)
            if (c0 + d < c1) { load_w(wr[d], c0 + d); stage_x(c0 + d, d); }
        int buf = 0;
        for (int c = c0; c < c1; c += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (c + d < c1) { phase(wr[d], c + d, buf); buf = buf == NB - 1 ? 0 : buf + 1; }
        }
    }
    // C layout of mfma_16x16: lane holds rows 4g + r of column n; the block scales went in with the FMAs
#pragma unroll
    for (int mt = 0; mt < RT; mt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = 16 * mt + 4 * g + r;
            const float v = acc[mt][r];
            if (out) out[(size_t)m * N + n0 + n] = (E)v;
            else __hip_atomic_store(&partial[((size_t)split * R + m) * N + n0 + n], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

extern "C" {

int samd_gemm_skinny_f8b(const void *d_A, const void *d_W8p, const float *d_sinv, int32_t rows_pad, int32_t N, int32_t K, int32_t splits, float *d_partial,
                         void *d_out, int32_t dtype, void *stream) {
    if (!d_A || !d_W8p || !d_sinv || ((uintptr_t)d_sinv & 7) != 0 || (rows_pad != 16 && rows_pad != 32 && rows_pad != 48 && rows_pad != 64) || N < GEMM_COLS ||
        N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0 || splits < 1 || splits > K / GEMM_KC || (splits == 1 ? !d_out : !d_partial) ||
        (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("samd_gemm_skinny_f8b: unsupported shape (rows 16/32/48/64, N %% 128 == 0, K %% 256 == 0, scale table 8-byte aligned) or null pointer");
        return SAMD_E_INVALID;
    }
    const dim3 grid(N / GEMM_COLS, splits);
    const hipStream_t st = (hipStream_t)stream;
    float *part = splits == 1 ? nullptr : d_partial;
    void *out = splits == 1 ? d_out : nullptr;
#define GO(TT, RT) e = stream_launch<k_gemm_skinny_f8b<TT, RT>, stream_lds(F8bDepth<RT>::value, RT)>(grid, st, (const typename TT::elem *)d_A, \
        (const unsigned char *)d_W8p, d_sinv, part, (typename TT::elem *)out, K, N, K / GEMM_KC, splits)
#define ROWS(TT) do { if (rows_pad == 16) GO(TT, 1); else if (rows_pad == 32) GO(TT, 2); else if (rows_pad == 48) GO(TT, 3); else GO(TT, 4); } while (0)
    hipError_t e;
    if (dtype == SAMD_F16) ROWS(GF16); else ROWS(GBF16);
#undef ROWS
#undef GO
    if (e != hipSuccess) { samd_set_error("samd_gemm_skinny_f8b: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"

// ================================================================================================
// Unpack: a quantised projection back to row-major [N][K] in the model dtype, straight from the buffer its streaming launch reads -- the
// inverses of samd_gemm_pack_f8 / _f4 / _i4 / _i8.  The one-pass prompt prefill of a quantised runner forms one projection at a time in a
// scratch matrix and hands it to the library product (samd_hip/llama.py: _prefill_wide); nothing is kept.
//   THE WEIGHTS are the ones the streaming launches multiply by, by construction: the widening is their device code -- W4Mx / W4Int's
//   group + cvt (F4Widen's v_cvt_scalef32_pk_*_fp4 with the block scale; I4Widen), I8Widen, F8Widen -- called on the same registers' worth
//   of a lane's unit, so MXFP4 is exact, INT4 / INT8 are rne_dtype((q - z) * s) with fp16 subnormals as v_pk_mul_f16 delivers them.  The
//   FP8 launches never form a weight (the scale goes on fp32 sums), so here the exact widened code goes to fp32, times the fp32 scale, and
//   is rounded ONCE to the model dtype: fp8.dequantize_rows / dequantize_blocks, then .to(dtype) -- one rounding per weight that the
//   decode step does not carry.
//   SHAPE: one 512-thread workgroup per packed block (tile t, chunk c), lane = the streaming kernels' lane (tid = 64 w + 16 g + n owns
//   row 128 t + 16 w + n).  Temporal 16-byte loads of the lane's units and one load of its side data; the widened units (a 16-code unit is
//   two, a 32-code unit four 16-byte pieces of its row) are staged in 64 KiB of LDS and leave as whole rows: every store instruction of a
//   wave writes the 512 contiguous bytes that two rows have in this chunk.  Measured against storing each lane's pieces directly (16
//   bytes per lane at a 32- or 64-byte stride, the line completed by the next one or three instructions): 22016 x 4096, fp16, 8-bit
//   51 - 56 -> 45 - 46 us, 4-bit 63 - 65 -> 38 - 40 us (profiles/quant_prefill.md), so the staging stays.  64 KiB of static LDS: two
//   workgroups per CU.  Plain vector loads and stores: capturable.
// ================================================================================================
enum { UNPACK_F8 = 0, UNPACK_F8B = 1, UNPACK_F4 = 2, UNPACK_I4 = 3, UNPACK_I8 = 4 };

// rne_dtype(float(v) * s) of 8 exactly widened FP8 codes
template <typename TT> struct UnpackScale;
template <> struct UnpackScale<GF16> {
    static __device__ __forceinline__ half8 mul(half8 v, float s) {
        half8 r;
#pragma unroll
        for (int i = 0; i < 8; i++) r[i] = (_Float16)((float)v[i] * s);
        return r;
    }
};
template <> struct UnpackScale<GBF16> {
    static __device__ __forceinline__ bf16x8 mul(bf16x8 v, float s) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float a = (float)v[2 * i] * s, b = (float)v[2 * i + 1] * s;
            unsigned p;
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(a), "v"(b));
            r[i] = p;
        }
        return __builtin_bit_cast(bf16x8, r);
    }
};

template <int F, typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES) void k_gemm_unpack(const unsigned char *__restrict__ Wp, const float *__restrict__ scale,
                                                                 typename TT::elem *__restrict__ out, int K, int n_chunks) {
    typedef typename TT::vec8 V;
    constexpr bool W4 = F == UNPACK_F4 || F == UNPACK_I4;
    constexpr size_t WCH = W4 ? 17408 : F == UNPACK_I8 ? 33792 : 32768, WU = 8192, WS = W4 ? 16384 : 32768;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, g = l >> 4;
    const int t = (int)(blockIdx.x / (unsigned)n_chunks), c = (int)(blockIdx.x - (unsigned)t * (unsigned)n_chunks);
    const unsigned char *blk = Wp + (size_t)blockIdx.x * WCH;
    const int row = GEMM_COLS * t + 16 * w + n;
    // the block's 64 KiB of output, [128 rows][32 units of 16 bytes]; unit u of row r sits at u ^ (r & 31), so the 16 rows of a wave's
    // ds_write_b128 and the 32 units of a row's read spread over all banks
    __shared__ __attribute__((aligned(16))) u32x4 stage[GEMM_COLS * 32];
    const int rl = 16 * w + n;
    auto put = [&](int kl, V v) { stage[rl * 32 + (((kl >> 3) ^ rl) & 31)] = __builtin_bit_cast(u32x4, v); };      // 8 weights at k = kl of this lane's row
    if constexpr (W4) {
        typedef typename std::conditional<F == UNPACK_F4, W4Mx, W4Int>::type Fmt;
        typename Fmt::side_t side;
        if constexpr (F == UNPACK_F4) side = *reinterpret_cast<const unsigned short *>(blk + WS + Fmt::slane(tid, w, n));
        else side = *reinterpret_cast<const u32x2 *>(blk + WS + Fmt::slane(tid, w, n));
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u32x4 u = *reinterpret_cast<const u32x4 *>(blk + WU * j + (size_t)tid * 16);
            const auto grp = Fmt::template group<TT>(side, j);
#pragma unroll
            for (int i = 0; i < 4; i++) put(128 * j + 32 * g + 8 * i, Fmt::template cvt<TT>(u[i], grp));      // the unit's 32 codes: k + 8 i .. + 7 in dword i
        }
    } else {
        u32x2 gd = {0u, 0u};
        float srow = 0.f;
        if constexpr (F == UNPACK_I8) gd = *reinterpret_cast<const u32x2 *>(blk + WS + (size_t)(16 * w + n) * 8);
        if constexpr (F == UNPACK_F8) srow = scale[row];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const u32x4 u = *reinterpret_cast<const u32x4 *>(blk + WU * b + (size_t)tid * 16);
            const int kl = 64 * b + 16 * g;                                   // the unit's 16 codes in k order
            if constexpr (F == UNPACK_I8) {
                const auto grp = I8Widen<TT>::group(gd, b >> 1);
                put(kl, I8Widen<TT>::cvt(u[0], u[1], grp));
                put(kl + 8, I8Widen<TT>::cvt(u[2], u[3], grp));
            } else {
                // block-scaled: the checkpoint's own table [N / 128][K / 128]; tile t is its row t, k block 2 c + (b >> 1)
                const float s = F == UNPACK_F8 ? srow : scale[(size_t)t * 2 * n_chunks + 2 * c + (b >> 1)];
                put(kl, UnpackScale<TT>::mul(F8Widen<TT>::cvt(u[0], u[1]), s));
                put(kl + 8, UnpackScale<TT>::mul(F8Widen<TT>::cvt(u[2], u[3]), s));
            }
        }
    }
    __syncthreads();
    // 32 consecutive lanes write the 512 contiguous bytes one row has in this chunk: every store instruction of a wave is two whole row pieces
    typename TT::elem *oblk = out + (size_t)GEMM_COLS * t * K + (size_t)c * GEMM_KC;
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const int u = it * 512 + tid, r = u >> 5, col = u & 31;
        *reinterpret_cast<u32x4 *>(oblk + (size_t)r * K + 8 * col) = stage[r * 32 + ((col ^ r) & 31)];
    }
}

// the checks and the launch of samd_gemm_unpack_*: everything is decided before any device work
template <int F>
static int gemm_unpack_call(const char *fn, const void *d_Wp, const float *d_scale, int N, int K, void *d_out, int dtype, void *stream) {
    constexpr bool scaled = F == UNPACK_F8 || F == UNPACK_F8B;
    if (!d_Wp || !d_out || d_Wp == d_out || (scaled && (!d_scale || (const void *)d_scale == d_out)) || (F == UNPACK_F8B && ((uintptr_t)d_scale & 7) != 0) ||
        (((uintptr_t)d_Wp | (uintptr_t)d_out) & 15) != 0 || N < GEMM_COLS || N % GEMM_COLS != 0 || K < GEMM_KC || K % GEMM_KC != 0 ||
        (long long)(N / GEMM_COLS) * (K / GEMM_KC) > 0x7fffffffLL || (dtype != SAMD_F16 && dtype != SAMD_BF16)) {
        samd_set_error("%s: needs N %% 128 == 0, K %% 256 == 0, dtype fp16 or bf16, 16-byte aligned distinct buffers%s", fn,
                       F == UNPACK_F8 ? " and a scale per row" : F == UNPACK_F8B ? " and an 8-byte aligned block-scale table" : "");
        return SAMD_E_INVALID;
    }
    const dim3 grid((unsigned)((N / GEMM_COLS) * (K / GEMM_KC)));
    if (dtype == SAMD_F16)
        hipLaunchKernelGGL((k_gemm_unpack<F, GF16>), grid, dim3(64 * GEMM_WAVES), 0, (hipStream_t)stream, (const unsigned char *)d_Wp, d_scale, (_Float16 *)d_out, K,
                           K / GEMM_KC);
    else
        hipLaunchKernelGGL((k_gemm_unpack<F, GBF16>), grid, dim3(64 * GEMM_WAVES), 0, (hipStream_t)stream, (const unsigned char *)d_Wp, d_scale, (__bf16 *)d_out, K,
                           K / GEMM_KC);
    LAUNCHCHK();
    return SAMD_OK;
}

extern "C" {

int samd_gemm_unpack_f8(const void *d_W8p, const float *d_scale, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    return gemm_unpack_call<UNPACK_F8>("samd_gemm_unpack_f8", d_W8p, d_scale, N, K, d_out, dtype, stream);
}

int samd_gemm_unpack_f8b(const void *d_W8p, const float *d_sinv, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    return gemm_unpack_call<UNPACK_F8B>("samd_gemm_unpack_f8b", d_W8p, d_sinv, N, K, d_out, dtype, stream);
}

int samd_gemm_unpack_f4(const void *d_W4p, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    return gemm_unpack_call<UNPACK_F4>("samd_gemm_unpack_f4", d_W4p, nullptr, N, K, d_out, dtype, stream);
}

int samd_gemm_unpack_i4(const void *d_W4p, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    return gemm_unpack_call<UNPACK_I4>("samd_gemm_unpack_i4", d_W4p, nullptr, N, K, d_out, dtype, stream);
}

int samd_gemm_unpack_i8(const void *d_W8p, int32_t N, int32_t K, void *d_out, int32_t dtype, void *stream) {
    return gemm_unpack_call<UNPACK_I8>("samd_gemm_unpack_i8", d_W8p, nullptr, N, K, d_out, dtype, stream);
}

}  // extern "C"

// ================================================================================================
// Mixture-of-experts MLP over MANY rows (a prompt in one pass): samd_moe_wide_route / _lists / _gate_up_silu / _down_combine serve 1 ..
// MOEW_MAX_ROWS rows (padded to 64 inside; rows >= *d_n route nowhere) with the kernels above.  An expert's list may now be longer than a
// 64-row tile, so the lists are followed by a TILE TABLE -- one record {expert, first entry, entries <= 64} per 64 entries of an expert's
// list, the tiles of one expert adjacent, experts ascending -- and an expert GEMM workgroup is moe_expert_gemm / moe8_expert_gemm<TT, 4,
// GU, WIDE = true> or gemm_stream_w4 / gemm_stream_i8<..., 4, ..., SIDE_WIDE, GU>: the 64-row tile's stream, MFMA sequence, epilogues and
// roundings, with `expert`, `cnt` and the list taken from its tile record instead of an active slot (moe_side_open).  A row's sum does not depend on the tile it sits in (chunk order over k, no
// split-K), so every row gets the bits the <= 64-row calls give it.
//   GRID (column tile, tile slot); the slot dimension is the shape's bound min(E, rows * k) + rows * k / 64 >= sum_e ceil(c_e / 64)
//   (each active expert has at most one partly filled tile); workgroups past ws[0] = the tile count exit at once.  Nothing comes back to
//   the host.  The row tiles of one expert are adjacent slots, 2 I / 128 or H / 128 workgroups apart in launch order: they run at about the
//   same time and meet the expert's weights in the L2 / Infinity Cache; nothing in the kernel enforces that (profiles/moe_prefill.md).
//   ROUTING WORKSPACE (int32 words at the head of d_ws, fixed offsets): [0] tiles; [1] active experts; [MOEW_WS_ACTIVE + a] expert of active
//   slot a (ascending); [MOEW_WS_COUNT + a] its entries; [MOEW_WS_OFFSET + a] its first entry's place in the entry array;
//   [MOEW_WS_TILE + 3 t ..] tile t's record; [MOEW_WS_ENTRY + i] the entries p = row * k + slot, expert by expert, ascending within an
//   expert, rows * k ints at most.  The down products y [rows_pad * k][hidden] follow at the next multiple of 256 bytes.
//   k_wmoe_lists: one workgroup per expert.  Every workgroup counts the entries of ALL experts (an LDS histogram: integer adds, the same
//   sums in any order), takes its own place from the counts of the experts below it, and writes its entries in ascending order by ballot
//   and prefix over 1024 entries at a time -- no atomic decides a position.  The ignore rules are k_moe_lists': rows >= *d_n, indices
//   outside [0, E), an expert repeated within a row.
// ================================================================================================
#define MOEW_LIST_THREADS 1024

__global__ __launch_bounds__(MOEW_LIST_THREADS) void k_wmoe_lists(const int *__restrict__ topk_idx, const int *__restrict__ d_n, int rows, int n_exp, int top_k, int *__restrict__ ws) {
    __shared__ int hist[MOE_MAX_E];
    __shared__ int wave_cnt[MOEW_LIST_THREADS / 64];
    const int tid = threadIdx.x, own = blockIdx.x, total = rows * top_k;
    int n = d_n[0];
    n = n < 0 ? 0 : (n > rows ? rows : n);
    if (tid < MOE_MAX_E) hist[tid] = 0;
    __syncthreads();
    auto expert_of = [&](int p) {
        const int r = p / top_k;
        int e = r < n ? topk_idx[p] : -1;
        if (e >= n_exp) e = -1;
        for (int q = r * top_k; q < p; q++) if (topk_idx[q] == e) e = -1;        // an expert counts once per row: its first slot
        return e;
    };
    for (int p = tid; p < total; p += MOEW_LIST_THREADS) {
        const int e = expert_of(p);
        if (e >= 0) atomicAdd(&hist[e], 1);
    }
    __syncthreads();
    int a = 0, off = 0, t0 = 0;                                  // active experts, entries and tiles below this expert
    for (int e = 0; e < own; e++) { const int c = hist[e]; a += c > 0; off += c; t0 += (c + MOE_MAX_ROWS - 1) / MOE_MAX_ROWS; }
    const int c = hist[own], nt = (c + MOE_MAX_ROWS - 1) / MOE_MAX_ROWS;
    if (own == n_exp - 1 && tid < 2) ws[tid] = tid == 0 ? t0 + nt : a + (c > 0);
    if (c == 0) return;                                          // (uniform)
    if (tid < 3) ws[(tid == 0 ? MOEW_WS_ACTIVE : tid == 1 ? MOEW_WS_COUNT : MOEW_WS_OFFSET) + a] = tid == 0 ? own : tid == 1 ? c : off;
    for (int t = tid; t < nt; t += MOEW_LIST_THREADS) {
        int *rec = ws + MOEW_WS_TILE + MOEW_TILE_INTS * (t0 + t);
        rec[0] = own; rec[1] = off + MOE_MAX_ROWS * t; rec[2] = c - MOE_MAX_ROWS * t < MOE_MAX_ROWS ? c - MOE_MAX_ROWS * t : MOE_MAX_ROWS;
    }
    int base = 0;
    for (int p0 = 0; p0 < total; p0 += MOEW_LIST_THREADS) {
        const int p = p0 + tid;
        const bool mine = p < total && expert_of(p) == own;
        const unsigned long long m = __ballot(mine);
        if ((tid & 63) == 0) wave_cnt[tid >> 6] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < MOEW_LIST_THREADS / 64; w++) { const int v = wave_cnt[w]; before += w < (tid >> 6) ? v : 0; all += v; }
        const int at = base + before + __popcll(m & ((1ull << (tid & 63)) - 1ull));
        if (mine && at < c) ws[MOEW_WS_ENTRY + off + at] = p;
        base += all;
        __syncthreads();
    }
}

template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe_gu(const typename TT::elem *__restrict__ h, const typename TT::elem *__restrict__ W, const int *__restrict__ ws,
                                                               typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    moe_expert_gemm<TT, 4, true, true>(h, W, ws, act, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe_dn(const typename TT::elem *__restrict__ act, const typename TT::elem *__restrict__ W, const int *__restrict__ ws,
                                                               typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    moe_expert_gemm<TT, 4, false, true>(act, W, ws, y, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe4_gu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W4, const int *__restrict__ ws,
                                                                typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Mx, TT, 4, MoeW4Depth<4>::value, SIDE_WIDE, true>(h, W4, ws, nullptr, act, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe4_dn(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W4, const int *__restrict__ ws,
                                                                typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Mx, TT, 4, MoeW4Depth<4>::value, SIDE_WIDE, false>(act, W4, ws, nullptr, y, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe_i4_gu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W4, const int *__restrict__ ws,
                                                                  typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Int, TT, 4, MoeW4Depth<4>::value, SIDE_WIDE, true>(h, W4, ws, nullptr, act, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 2) void k_wmoe_i4_dn(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W4, const int *__restrict__ ws,
                                                                  typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    gemm_stream_w4<W4Int, TT, 4, MoeW4Depth<4>::value, SIDE_WIDE, false>(act, W4, ws, nullptr, y, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 1) void k_wmoe8_gu(const typename TT::elem *__restrict__ h, const unsigned char *__restrict__ W8, const float *__restrict__ stab,
                                                                const int *__restrict__ ws, typename TT::elem *__restrict__ act, int K, int N, int n_chunks, int top_k) {
    moe8_expert_gemm<TT, 4, true, true>(h, W8, stab, ws, act, K, N, n_chunks, top_k);
}
template <typename TT>
__global__ __launch_bounds__(64 * GEMM_WAVES, 1) void k_wmoe8_dn(const typename TT::elem *__restrict__ act, const unsigned char *__restrict__ W8, const float *__restrict__ stab,
                                                                const int *__restrict__ ws, typename TT::elem *__restrict__ y, int K, int N, int n_chunks, int top_k) {
    moe8_expert_gemm<TT, 4, false, true>(act, W8, stab, ws, y, K, N, n_chunks, top_k);
}

// one wide expert launch: the format's kernel at the 64-row tile with that tile's dynamic LDS, grid (N / 128, tile slots)
template <typename TT, bool GU>
static hipError_t wmoe_gemm_format(int fmt, dim3 grid, hipStream_t st, const void *A, const void *W, size_t w_rows, const int *ws, void *out, int K, int N, int top_k) {
    typedef typename TT::elem E;
    const unsigned char *wb = (const unsigned char *)W;
    const int nc = K / GEMM_KC;
    if (fmt == 0) return stream_launch<(GU ? k_wmoe_gu<TT> : k_wmoe_dn<TT>), stream_lds(2, 4)>(grid, st, (const E *)A, (const E *)W, ws, (E *)out, K, N, nc, top_k);
    if (fmt == 1) return stream_launch<(GU ? k_wmoe4_gu<TT> : k_wmoe4_dn<TT>), stream_lds(MoeW4Depth<4>::value, 4)>(grid, st, (const E *)A, wb, ws, (E *)out, K, N, nc, top_k);
    if (fmt == 2) return stream_launch<(GU ? k_wmoe_i4_gu<TT> : k_wmoe_i4_dn<TT>), stream_lds(MoeW4Depth<4>::value, 4)>(grid, st, (const E *)A, wb, ws, (E *)out, K, N, nc, top_k);
    if (fmt == 5) return stream_launch<(GU ? k_moew_i8_gu<TT> : k_moew_i8_dn<TT>), stream_lds(MoeI8Depth<4>::value, 4)>(grid, st, (const E *)A, wb, ws, (E *)out, K, N, nc, top_k);
    const float *stab = reinterpret_cast<const float *>(reinterpret_cast<const char *>(W) + moe8_scale_offset(w_rows, (size_t)K));
    return stream_launch<(GU ? k_wmoe8_gu<TT> : k_wmoe8_dn<TT>), stream_lds(Moe8Depth<4>::value, 4)>(grid, st, (const E *)A, wb, stab, ws, (E *)out, K, N, nc, top_k);
}

static inline int moew_rows_pad(int rows) { return (rows + MOE_MAX_ROWS - 1) / MOE_MAX_ROWS * MOE_MAX_ROWS; }
static inline int64_t moew_y_off(int rows_pad, int top_k) { return (((int64_t)MOEW_WS_ENTRY + (int64_t)rows_pad * top_k) * 4 + 255) / 256 * 256; }
// the tile slots of a launch: every active expert has at most one partly filled tile
static inline int moew_tile_bound(int rows_pad, int n_experts, int top_k) {
    const int total = rows_pad * top_k;
    return (n_experts < total ? n_experts : total) + total / MOE_MAX_ROWS;
}
// the checks shared by the wide calls, in the order the messages promise; sets the error text
static bool moew_args_ok(const char *fn, bool pointers, int rows, int hidden, int moe_inter, int n_experts, int top_k, int dtype, int fmt) {
    if (rows < 1 || rows > MOEW_MAX_ROWS) { samd_set_error("%s: rows %d outside 1 .. %d", fn, rows, MOEW_MAX_ROWS); return false; }
    if (fmt < 0 || fmt > 5 || fmt == 4) {                        // (4 is left unassigned: callers pin it as an unknown code)
        samd_set_error("%s: unknown expert_format %d (0 model dtype, 1 mxfp4, 2 int4g128, 3 fp8b128, 5 int8g128)", fn, fmt); return false;
    }
    if (!moe_shape_ok(MOE_MAX_ROWS, hidden, moe_inter, n_experts, top_k, dtype) || (fmt == 3 && (hidden > 128 * MOE8_MAX_KB || moe_inter > 128 * MOE8_MAX_KB))) {
        samd_set_error("%s: unsupported shape (hidden %% 256 == 0, moe_intermediate %% 256 == 0, both <= 16384 for fp8b128, experts <= 256, top-k <= 8, f16/bf16)", fn);
        return false;
    }
    if (!pointers) { samd_set_error("%s: null pointer", fn); return false; }
    return true;
}

extern "C" {

int64_t samd_moe_wide_workspace_layout(int32_t field, int32_t rows, int32_t top_k) {
    const int rp = moew_rows_pad(rows < 1 ? 1 : rows);
    switch (field) {
    case 0: return MOEW_WS_ACTIVE;
    case 1: return MOEW_WS_COUNT;
    case 2: return MOEW_WS_OFFSET;
    case 3: return MOEW_WS_TILE;
    case 4: return MOEW_TILE_INTS;
    case 5: return MOEW_WS_ENTRY;
    case 6: return (int64_t)MOEW_WS_ENTRY + (int64_t)rp * top_k;       // int32 words of the routing part
    case 7: return moew_y_off(rp, top_k);                               // byte offset of the down products
    case 8: return MOEW_MAX_ROWS;
    case 9: return MOEW_MAX_TILES;
    default: return -1;
    }
}

int64_t samd_moe_wide_workspace(int32_t rows, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, int32_t dtype) {
    if (!moew_args_ok("samd_moe_wide_workspace", true, rows, hidden, moe_inter, n_experts, top_k, dtype, 0)) return SAMD_E_INVALID;
    const int rp = moew_rows_pad(rows);
    return moew_y_off(rp, top_k) + (int64_t)rp * top_k * hidden * 2;
}

int samd_moe_wide_route(const void *d_h, const void *d_router, const int32_t *d_n, int32_t rows, int32_t hidden, int32_t n_experts, int32_t top_k, int32_t norm_topk,
                        int32_t *d_topk_idx, void *d_topk_w, int32_t dtype, void *stream) {
    if (!moew_args_ok("samd_moe_wide_route", d_h && d_router && d_n && d_topk_idx && d_topk_w, rows, hidden, GEMM_KC, n_experts, top_k, dtype, 0)) return SAMD_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int rp = moew_rows_pad(rows);
    if (dtype == SAMD_F16)
        hipLaunchKernelGGL(k_moe_route<_Float16>, dim3(rp), dim3(64 * MOE_ROUTE_WAVES), 0, st, (const _Float16 *)d_h, (const _Float16 *)d_router, d_n, hidden, n_experts, top_k, norm_topk,
                           d_topk_idx, (_Float16 *)d_topk_w);
    else
        hipLaunchKernelGGL(k_moe_route<__bf16>, dim3(rp), dim3(64 * MOE_ROUTE_WAVES), 0, st, (const __bf16 *)d_h, (const __bf16 *)d_router, d_n, hidden, n_experts, top_k, norm_topk,
                           d_topk_idx, (__bf16 *)d_topk_w);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_wide_lists(const int32_t *d_topk_idx, const int32_t *d_n, int32_t rows, int32_t n_experts, int32_t top_k, void *d_ws, void *stream) {
    if (!moew_args_ok("samd_moe_wide_lists", d_topk_idx && d_n && d_ws, rows, GEMM_KC, GEMM_KC, n_experts, top_k, SAMD_F16, 0)) return SAMD_E_INVALID;
    hipLaunchKernelGGL(k_wmoe_lists, dim3(n_experts), dim3(MOEW_LIST_THREADS), 0, (hipStream_t)stream, d_topk_idx, d_n, moew_rows_pad(rows), n_experts, top_k, (int *)d_ws);
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_wide_gate_up_silu(const void *d_h, const void *d_Wgu, const void *d_ws, int32_t rows, int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k,
                               int32_t expert_format, void *d_act, int32_t dtype, void *stream) {
    if (!moew_args_ok("samd_moe_wide_gate_up_silu", d_h && d_Wgu && d_ws && d_act, rows, hidden, moe_inter, n_experts, top_k, dtype, expert_format)) return SAMD_E_INVALID;
    const dim3 grid(2 * moe_inter / GEMM_COLS, moew_tile_bound(moew_rows_pad(rows), n_experts, top_k));
    const size_t w_rows = (size_t)n_experts * 2 * moe_inter;
    const hipError_t e = dtype == SAMD_F16
        ? wmoe_gemm_format<GF16, true>(expert_format, grid, (hipStream_t)stream, d_h, d_Wgu, w_rows, (const int *)d_ws, d_act, hidden, 2 * moe_inter, top_k)
        : wmoe_gemm_format<GBF16, true>(expert_format, grid, (hipStream_t)stream, d_h, d_Wgu, w_rows, (const int *)d_ws, d_act, hidden, 2 * moe_inter, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_wide_gate_up_silu: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    return SAMD_OK;
}

int samd_moe_wide_down_combine(const void *d_act, const void *d_Wdown, const int32_t *d_topk_idx, const void *d_topk_w, const int32_t *d_n, void *d_ws, int32_t rows,
                               int32_t hidden, int32_t moe_inter, int32_t n_experts, int32_t top_k, int32_t expert_format, void *d_out, int32_t dtype, void *stream) {
    if (!moew_args_ok("samd_moe_wide_down_combine", d_act && d_Wdown && d_topk_idx && d_topk_w && d_n && d_ws && d_out, rows, hidden, moe_inter, n_experts, top_k, dtype,
                      expert_format)) return SAMD_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int rp = moew_rows_pad(rows);
    void *y = (char *)d_ws + moew_y_off(rp, top_k);
    const dim3 grid(hidden / GEMM_COLS, moew_tile_bound(rp, n_experts, top_k));
    const size_t w_rows = (size_t)n_experts * hidden;
    const hipError_t e = dtype == SAMD_F16
        ? wmoe_gemm_format<GF16, false>(expert_format, grid, st, d_act, d_Wdown, w_rows, (const int *)d_ws, y, moe_inter, hidden, top_k)
        : wmoe_gemm_format<GBF16, false>(expert_format, grid, st, d_act, d_Wdown, w_rows, (const int *)d_ws, y, moe_inter, hidden, top_k);
    if (e != hipSuccess) { samd_set_error("samd_moe_wide_down_combine: %s", hipGetErrorString(e)); return SAMD_E_HIP; }
    LAUNCHCHK();
    moe_combine_launch(dtype, st, y, d_topk_idx, d_topk_w, d_n, d_out, rp, hidden, top_k, n_experts);
    LAUNCHCHK();
    return SAMD_OK;
}

}  // extern "C"
