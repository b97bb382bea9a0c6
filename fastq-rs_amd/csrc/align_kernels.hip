// align_kernels.hip — per-record Smith-Waterman-Gotoh local alignment scores against one query (fqh_align_scores): the
// closure of the crate's alignment example (examples/alignment_count.rs:19-36, src/lib.rs:78-91) for every record at once.
//
// One record per lane.  The query's rows run down the lane's registers: HG[i] = H[i][j-1] - gap_open and E[i] of the
// previous column, 2 x ROWS VGPRs; the read streams through as columns, one byte per column, and F is one value carried
// down the column.  The query is wave-uniform: the block builds, from the kernel arguments, a 256-entry table in LDS whose
// entry c holds s(q_i, c) + gap_open for every row i as packed int16 — the column's match pattern is ROWS/2 dwords read
// once per column (ds_read_b128), and the cell adds its half-word (an SDWA operand).  Per cell then (ISA):
//   d  = HG[i-1]_old + t_i          H[i-1][j-1] + s  (t_i = s + gap_open, HG = H - gap_open)
//   e  = max(E[i] - ge, HG[i]_old)  E[i][j]
//   f  = max(f - ge, hg_up, 0)      F[i][j] clamped at 0, which changes no H (H = max(0, ...) anyway) and saves the 0 below
//   h  = max(d, e, f)               H[i][j]
//   hg = h - gap_open               for E of the next column and F / the diagonal of the next row
// plus one max3 per two cells for the column's maximum.
//
// Short queries: the kernel is instantiated for ROWS = 16, 32, 64 and a query of m < ROWS bytes occupies the LAST m rows.
// The first ROWS - m rows carry t = 0: their H stays 0 (d = -gap_open + 0 <= 0, E and F <= 0 there) and what they pass down
// (HG = -gap_open, f = 0) is exactly the row-0 boundary (H = 0, F = -inf clamped at 0), so they change no score or end.
//
// Every loop is bounded: the column loop by the record's own seq() length from the index, the rows by ROWS.
#include <hip/hip_runtime.h>

#include "fqh_internal.h"

namespace fqh {

struct AlignQuery {
    uint32_t qw[16];    // row r's query byte in byte r % 4 of qw[r / 4] (rows already placed: the query fills the last rows)
    uint64_t real;      // bit r: row r holds a query byte (0: padding row)
    int32_t t_match;    // match + gap_open
    int32_t t_mismatch; // mismatch + gap_open
    int32_t go, ge, threshold;
};

constexpr int32_t NEG_INF = -(1 << 20);  // E's boundary: the first column lifts it to >= -gap_open; never near overflow

template <int ROWS>
__global__ __launch_bounds__(256) void k_align(const uint8_t *__restrict__ buf, uint64_t base_offset,
                                               const fqh_idx_record *__restrict__ idx, uint64_t n, AlignQuery q,
                                               int32_t *__restrict__ out_score, uint32_t *__restrict__ out_end,
                                               uint8_t *__restrict__ flags, unsigned long long *__restrict__ count) {
    constexpr int NW = ROWS / 2;  // packed int16 pairs per table entry
    __shared__ __attribute__((aligned(16))) uint32_t tab[256 * NW];
    __shared__ uint32_t block_hits[4];
    {
        // thread c builds entry c: every row index below is a compile-time constant (query bytes stay in SGPRs)
        const uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            uint32_t pair = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = 2 * k + h;
                const uint32_t qb = (q.qw[r >> 2] >> (8 * (r & 3))) & 0xFFu;
                const int32_t t = ((q.real >> r) & 1) ? (qb == c ? q.t_match : q.t_mismatch) : 0;
                pair |= ((uint32_t)t & 0xFFFFu) << (16 * h);
            }
            tab[c * NW + k] = pair;
        }
    }
    __syncthreads();

    const uint64_t rec = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t best = 0;
    uint32_t end = 0xFFFFFFFFu;
    if (rec < n) {
        const fqh_idx_record r = idx[rec];
        // first sequence byte relative to buf; negative for a record that began in the caller's lead area
        const uint8_t *p = buf + (int64_t)(r.start - base_offset) + r.head + 1;
        uint32_t sl = r.seq - r.head - 1;
        if (sl && p[sl - 1] == '\r') --sl;  // trim_winline, src/records.rs:66-73
        const int32_t go = q.go, ge = q.ge;
        int32_t HG[ROWS], E[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            HG[i] = -go;  // H[i][0] = 0
            E[i] = NEG_INF;
        }
        uint32_t w = 0;
        for (uint32_t j = 0; j < sl; ++j) {
            // dword loads from the sequence line: a dword starting at j < sl ends at most 3 bytes past the line, which are
            // still inside the record ('\n', the '+' line and its '\n' follow every complete record's sequence)
            if ((j & 3u) == 0) __builtin_memcpy(&w, p + j, 4);
            const uint32_t c = w & 0xFFu;
            w >>= 8;
            uint32_t t[NW];
            const uint4 *row = reinterpret_cast<const uint4 *>(&tab[c * NW]);
#pragma unroll
            for (int k = 0; k < NW / 4; ++k) {
                const uint4 v = row[k];
                t[4 * k] = v.x; t[4 * k + 1] = v.y; t[4 * k + 2] = v.z; t[4 * k + 3] = v.w;
            }
            int32_t diag = -go;   // HG of row -1 at column j-1 (boundary H = 0)
            int32_t hg_up = -go;  // HG of the row above at column j
            int32_t f = 0;        // F of the row above, clamped at 0 (boundary -inf)
            int32_t cmax = 0;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const int32_t ti = (int32_t)(int16_t)(t[i >> 1] >> (16 * (i & 1)));
                const int32_t d = diag + ti;
                const int32_t e = max(E[i] - ge, HG[i]);
                f = max(max(f - ge, hg_up), 0);
                const int32_t h = max(max(d, e), f);
                diag = HG[i];
                hg_up = h - go;
                HG[i] = hg_up;
                E[i] = e;
                cmax = max(cmax, h);
            }
            if (cmax > best) {  // strict: the first column that reaches the score names the end
                best = cmax;
                end = j;
            }
        }
        if (out_score) out_score[rec] = best;
        if (out_end) out_end[rec] = end;
        if (flags) flags[rec] = (uint8_t)((flags[rec] & ~FQH_FLAG_ADAPTER) | (best > q.threshold ? FQH_FLAG_ADAPTER : 0u));
    }
    if (count) {
        const unsigned long long hit = __ballot(rec < n && best > q.threshold);
        if ((threadIdx.x & 63u) == 0) block_hits[threadIdx.x >> 6] = (uint32_t)__popcll(hit);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t s = block_hits[0] + block_hits[1] + block_hits[2] + block_hits[3];
            if (s) atomicAdd(count, (unsigned long long)s);
        }
    }
}

uint32_t align_rows(uint32_t query_len) { return query_len <= 16 ? 16u : query_len <= 32 ? 32u : 64u; }

void launch_align(hipStream_t s, const uint8_t *buf, uint64_t base_offset, const fqh_idx_record *idx, uint64_t n,
                  const uint8_t *query, uint32_t query_len, int32_t match, int32_t mismatch, int32_t gap_open,
                  int32_t gap_extend, int32_t threshold, int32_t *score, uint32_t *end, uint8_t *flags,
                  unsigned long long *count) {
    if (!n) return;
    const uint32_t rows = align_rows(query_len);
    AlignQuery q{};
    const uint32_t pad = rows - query_len;
    for (uint32_t i = 0; i < query_len; ++i) {
        const uint32_t r = pad + i;
        q.qw[r >> 2] |= (uint32_t)query[i] << (8 * (r & 3));
        q.real |= 1ull << r;
    }
    q.t_match = match + gap_open;
    q.t_mismatch = mismatch + gap_open;
    q.go = gap_open;
    q.ge = gap_extend;
    q.threshold = threshold;
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    if (rows == 16)
        hipLaunchKernelGGL(k_align<16>, grid, block, 0, s, buf, base_offset, idx, n, q, score, end, flags, count);
    else if (rows == 32)
        hipLaunchKernelGGL(k_align<32>, grid, block, 0, s, buf, base_offset, idx, n, q, score, end, flags, count);
    else
        hipLaunchKernelGGL(k_align<64>, grid, block, 0, s, buf, base_offset, idx, n, q, score, end, flags, count);
}

}  // namespace fqh
