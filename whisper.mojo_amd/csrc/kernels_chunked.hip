// kernels_chunked.hip — the stitch of chunked long-form transcription: per recording, the id lists of its overlapping
// chunks, in chunk order, merged as HF's tokenization_whisper._find_longest_common_sequence(sequences) merges them (the form without
// token timestamps), after the strip of _decode_asr: every id >= first_special is dropped, and a chunk that keeps no id is no operand.
//
// One workgroup per recording.  `left` is the remainder of the previous merge, so the operands are walked serially; inside one merge
// the candidate offsets i = 1 .. L + R - 1 are spread over the threads.  The score matches / i + i / 10000.0 is formed in float64
// with the operations Python performs (one division, one division, one addition: all correctly rounded), so the comparison is HF's
// bit for bit; a candidate counts only with matches > 1, and the strict maximum in ascending i means the lowest i wins a tie.
#include "wm_kernels.h"

namespace wm {

static const int CM_THREADS = 256;

// rows[k] = [n, ids ...] (1 + stride ints), the packed rows pack_tokens_kernel writes; recording r owns rows [rec_off[r], rec_off[r + 1]).
// LDS: left[stride], right[stride] (dynamic), the reduction's 256 (score, i) pairs and the compaction's wave counts.
__global__ __launch_bounds__(CM_THREADS) void chunk_merge_kernel(const int* __restrict__ rows, const int* __restrict__ rec_off, int stride,
                                                                 int first_special, int* __restrict__ merged, int* __restrict__ merged_len,
                                                                 int cap) {
    extern __shared__ int s_ids[];
    __shared__ double s_score[CM_THREADS];
    __shared__ int s_best[CM_THREADS];
    __shared__ int s_wcnt[CM_THREADS / 64];
    int* left = s_ids;
    int* right = s_ids + stride;
    const int tid = threadIdx.x, rec = blockIdx.x;
    const int k0 = rec_off[rec], k1 = rec_off[rec + 1];
    int* out = merged + (size_t)rec * cap;
    int L = 0, total = 0;
    bool have_left = false;
    for (int k = k0; k < k1; ++k) {
        const int* row = rows + (size_t)k * (1 + stride);
        const int n = min(max(row[0], 0), stride);
        // the strip, order kept: ballot per wave, the waves' counts through LDS
        int R = 0;
        for (int base = 0; base < n; base += CM_THREADS) {
            const int j = base + tid;
            const int id = j < n ? row[1 + j] : -1;
            const bool keep = j < n && id >= 0 && id < first_special;
            const unsigned long long mask = __ballot(keep);
            const int lane = tid & 63, wave = tid >> 6;
            if (lane == 0) s_wcnt[wave] = __popcll(mask);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < CM_THREADS / 64; ++w) {
                if (w < wave) before += s_wcnt[w];
                all += s_wcnt[w];
            }
            if (keep) right[R + before + __popcll(mask & ((1ull << lane) - 1ull))] = id;
            R += all;
            __syncthreads();
        }
        if (R == 0) continue;  // `if current_tokens:` — an empty chunk is no operand
        if (!have_left) {      // sequences[0]
            for (int j = tid; j < R; j += CM_THREADS) left[j] = right[j];
            L = R;
            have_left = true;
            __syncthreads();
            continue;
        }
        // every thread's best candidate, ascending i with a strict maximum
        double best = 0.0;
        int best_i = 0x7fffffff;
        for (int i = 1 + tid; i < L + R; i += CM_THREADS) {
            const int ls = max(0, L - i), le = min(L, L + R - i), rs = max(0, i - L);
            int matches = 0;
            for (int j = 0; j < le - ls; ++j) matches += left[ls + j] == right[rs + j];
            const double sc = (double)matches / (double)i + (double)i / 10000.0;
            if (matches > 1 && sc > best) {
                best = sc;
                best_i = i;
            }
        }
        s_score[tid] = best;
        s_best[tid] = best_i;
        __syncthreads();
        for (int s = CM_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const double o = s_score[tid + s];
                const int oi = s_best[tid + s];
                const bool take = o > s_score[tid] || (o == s_score[tid] && oi < s_best[tid]);
                if (take) {
                    s_score[tid] = o;
                    s_best[tid] = oi;
                }
            }
            __syncthreads();
        }
        const int bi = s_best[0];
        // max_indices: HF's default (L, L, 0, 0) when nothing matched is plain concatenation
        int ls = L, le = L, rs = 0, re = 0;
        if (bi != 0x7fffffff) {
            ls = max(0, L - bi);
            le = min(L, L + R - bi);
            rs = max(0, bi - L);
            re = min(R, bi);
        }
        const int left_mid = (le + ls) / 2, right_mid = (re + rs) / 2;
        for (int j = tid; j < left_mid; j += CM_THREADS)
            if (total + j < cap) out[total + j] = left[j];
        total += left_mid;
        __syncthreads();  // everyone is done reading left
        L = R - right_mid;
        for (int j = tid; j < L; j += CM_THREADS) left[j] = right[right_mid + j];
        __syncthreads();
    }
    for (int j = tid; j < L; j += CM_THREADS)
        if (total + j < cap) out[total + j] = left[j];
    total += L;
    if (tid == 0) merged_len[rec] = min(total, cap);
}

size_t chunk_merge_lds_bytes(int stride) { return (size_t)2 * stride * sizeof(int); }

int launch_chunk_merge(const int* rows, const int* rec_off, int n_rec, int stride, int first_special, int* merged, int* merged_len, int cap,
                       hipStream_t st) {
    if (n_rec <= 0 || stride <= 0 || cap <= 0) return launch_refuse("chunk_merge: recordings, ids per row and output capacity must be positive");
    if (stride > CHUNK_MERGE_MAX_IDS) return launch_refuse("chunk_merge: more ids per row than the kernel's LDS holds (CHUNK_MERGE_MAX_IDS = 2048)");
    hipLaunchKernelGGL(chunk_merge_kernel, dim3(n_rec), dim3(CM_THREADS), chunk_merge_lds_bytes(stride), st, rows, rec_off, stride, first_special,
                       merged, merged_len, cap);
    return hipGetLastError() == hipSuccess ? WM_LAUNCH_OK : WM_LAUNCH_HIP;
}

}  // namespace wm
