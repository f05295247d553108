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

// ---- the stitch with timestamps ---------------------------------------------------------------------------------------
// HF's tokenization_whisper._decode_asr with return_timestamps = True ("segments") or "word": the state machine that walks each
// chunk's ids, skips the timestamp ids that fall inside a stride, closes a segment at an end timestamp, and at every close merges the
// operands gathered since the last one with _find_longest_common_sequence(previous_tokens, previous_token_timestamps).  That merge is
// a left fold — total_sequence is only ever extended — so it is folded here as the operands arrive: `left` is what the fold has not
// emitted yet, always a piece of ONE row, and the emitted ids go straight to the output.  One workgroup per recording; the walk is
// serial and uniform over the workgroup (every thread computes the same scalars), the strip of an operand and the candidate offsets
// of a merge are spread over the threads as in chunk_merge_kernel.  chunk_merge_kernel itself is left as it is: this search carries
// a position per id and, in word mode, the pair comparison, which would change that kernel's registers.
//
// Times are float64, formed with the operations Python performs in Python's order; products and sums go through __dmul_rn /
// __dadd_rn so that none contracts into an FMA.

// Python's round(x, 2): the double nearest to the correctly rounded two-decimal value of x's exact binary value.  c = rint(100 |x|)
// is at most one off; |x| = m · 2^-s exactly, so 200 |x| = 200 m / 2^s is compared with the half-way points (2c ± 1) in 64-bit
// integers (200 · 2^53 < 2^63), an exact tie going to the even c.  From 2^46 on the doubles lie further apart than 0.01 and x is
// its own answer; below 2^-10 the answer is a zero with x's sign.
__device__ double py_round2(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const int E = (int)((b >> 52) & 0x7ff);
    if (E >= 1023 + 46) return x;  // (inf and nan included)
    const int s = 1075 - E;
    if (E == 0 || s > 62) return copysign(0.0, x);
    const unsigned long long m = (b & 0xfffffffffffffULL) | (1ULL << 52);
    unsigned long long c = (unsigned long long)rint(__dmul_rn(fabs(x), 100.0));
    const unsigned long long T = 200ULL * m;
    const unsigned long long hi = (2ULL * c + 1ULL) << s;
    if (T > hi || (T == hi && (c & 1ULL))) {
        ++c;
    } else if (c > 0) {
        const unsigned long long lo = (2ULL * c - 1ULL) << s;
        if (T < lo || (T == lo && (c & 1ULL))) --c;
    }
    return copysign(__ddiv_rn((double)c, 100.0), x);
}

// the (start, end) pair of the id at position i of a row whose token times are tt, under that chunk's time_offset
__device__ inline void cs_pair(const float* __restrict__ tt, int i, double off, double& s, double& e) {
    s = py_round2(__dadd_rn(i == 0 ? 0.0 : (double)tt[i - 1], off));
    e = py_round2(__dadd_rn((double)tt[i], off));
}

__global__ __launch_bounds__(CM_THREADS) void chunk_segments_kernel(const ChunkSegArgs a) {
    extern __shared__ int s_ids[];
    __shared__ double s_score[CM_THREADS];
    __shared__ int s_best[CM_THREADS];
    __shared__ int s_wcnt[CM_THREADS / 64];
    const int stride = a.stride;
    int* left = s_ids;                  // ids the fold has not emitted yet ...
    int* left_pos = s_ids + stride;     // ... and their positions in row left_row
    int* right = s_ids + 2 * stride;
    int* right_pos = s_ids + 3 * stride;
    const int tid = threadIdx.x, rec = blockIdx.x;
    const int k0 = a.rec_off[rec], k1 = a.rec_off[rec + 1];
    const bool word = a.times != nullptr;
    const int tb = a.timestamp_begin, cap = a.cap;
    const double tp = a.time_precision;
    int* out = a.merged + (size_t)rec * cap;
    double* out_pairs = word ? a.pairs + (size_t)rec * cap * 2 : nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // what persists across chunks
    double time_offset = 0.0, start = nan;
    bool skip = false, have_start = false, any_ids = false;
    int n_ops = 0;                      // len(previous_tokens)
    int L = 0, left_row = 0;            // the fold's remainder: L ids of row left_row, heard under left_off
    double left_off = 0.0;
    int total = 0, seg_first = 0, nseg = 0;

    // left[0 .. n) -> the output, ids and (word mode) pairs
    auto emit = [&](int n) {
        const float* tt = word ? a.times + (size_t)left_row * stride : nullptr;
        for (int j = tid; j < n; j += CM_THREADS)
            if (total + j < cap) {
                out[total + j] = left[j];
                if (word) {
                    double s, e;
                    cs_pair(tt, left_pos[j], left_off, s, e);
                    out_pairs[2 * (size_t)(total + j)] = s;
                    out_pairs[2 * (size_t)(total + j) + 1] = e;
                }
            }
        total += n;
    };
    // the text ids of row[b .. e) -> right / right_pos, order kept: ballot per wave, the waves' counts through LDS
    auto strip = [&](const int* row, int b, int e) {
        int R = 0;
        for (int base = b; base < e; base += CM_THREADS) {
            const int j = base + tid;
            const int id = j < e ? row[1 + j] : a.first_special;
            const bool keep = j < e && id < a.first_special;
            const unsigned long long mask = __ballot(keep);
            const int lane = tid & 63, wave = tid >> 6;
            if (lane == 0) s_wcnt[wave] = __popcll(mask);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < CM_THREADS / 64; ++w) {
                if (w < wave) before += s_wcnt[w];
                all += s_wcnt[w];
            }
            if (keep) {
                const int at = R + before + __popcll(mask & ((1ull << lane) - 1ull));
                right[at] = id;
                right_pos[at] = j;
            }
            R += all;
            __syncthreads();
        }
        return R;
    };
    // previous_tokens.append(right): the first operand becomes `left`, every later one is merged into it
    auto operand = [&](int R, int k, double off) {
        if (n_ops > 0) {
            const float* ltt = word ? a.times + (size_t)left_row * stride : nullptr;
            const float* rtt = word ? a.times + (size_t)k * stride : nullptr;
            double best = 0.0;
            int best_i = 0x7fffffff;
            for (int i = 1 + tid; i < L + R; i += CM_THREADS) {
                const int ls = max(0, L - i), le = min(L, L + R - i), rs = max(0, i - L);
                int matches = 0;
                for (int j = 0; j < le - ls; ++j) {
                    if (left[ls + j] != right[rs + j]) continue;
                    if (word) {  // ... and the left pair <= the right pair, as Python compares tuples
                        double s0, e0, s1, e1;
                        cs_pair(ltt, left_pos[ls + j], left_off, s0, e0);
                        cs_pair(rtt, right_pos[rs + j], off, s1, e1);
                        if (!(s0 < s1 || (s0 == s1 && e0 <= e1))) continue;
                    }
                    ++matches;
                }
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
                    if (o > s_score[tid] || (o == s_score[tid] && oi < s_best[tid])) {
                        s_score[tid] = o;
                        s_best[tid] = oi;
                    }
                }
                __syncthreads();
            }
            const int bi = s_best[0];
            int ls = L, le = L, rs = 0, re = 0;  // HF's default: plain concatenation
            if (bi != 0x7fffffff) {
                ls = max(0, L - bi);
                le = min(L, L + R - bi);
                rs = max(0, bi - L);
                re = min(R, bi);
            }
            const int left_mid = (le + ls) / 2, right_mid = (re + rs) / 2;
            emit(left_mid);
            __syncthreads();  // everyone is done reading left
            L = R - right_mid;
            for (int j = tid; j < L; j += CM_THREADS) {
                left[j] = right[right_mid + j];
                left_pos[j] = right_pos[right_mid + j];
            }
        } else {
            L = R;
            for (int j = tid; j < L; j += CM_THREADS) {
                left[j] = right[j];
                left_pos[j] = right_pos[j];
            }
        }
        left_row = k;
        left_off = off;
        ++n_ops;
        any_ids = any_ids || R > 0;
        __syncthreads();
    };
    // chunks.append(chunk): the rest of the fold, then the segment's record
    auto flush = [&](double end) {
        emit(L);
        __syncthreads();
        L = 0;
        if (tid == 0 && nseg < a.seg_cap) {
            double* t = a.seg_times + ((size_t)rec * a.seg_cap + nseg) * 2;
            int* r = a.seg_range + ((size_t)rec * a.seg_cap + nseg) * 2;
            t[0] = have_start ? start : nan;
            t[1] = end;
            r[0] = min(seg_first, cap);
            r[1] = min(total, cap);
        }
        ++nseg;
        seg_first = total;
        n_ops = 0;
        any_ids = false;
        have_start = false;
    };

    for (int k = k0; k < k1; ++k) {
        const int* row = a.rows + (size_t)k * (1 + stride);
        const int n = min(max(row[0], 0), stride);
        const int* t3 = a.tab + (size_t)k * a.tab_cols + a.tab_c0;
        const double chunk_len = (double)t3[0] / 16000.0, stride_left = (double)t3[1] / 16000.0, stride_right = (double)t3[2] / 16000.0;
        time_offset = __dadd_rn(time_offset, -stride_left);
        const double right_start = __dadd_rn(chunk_len, -stride_right);
        const double first_timestamp = t3[1] != 0 ? __dadd_rn(stride_left / tp, (double)tb) : (double)tb;
        int last_timestamp = -1;  // None
        if (t3[2] != 0)
            for (int j = n - 1; j >= 0; --j) {
                const int t = row[1 + j];
                if (t < tb) continue;
                if (last_timestamp >= 0 && __dmul_rn((double)(t - tb), tp) < right_start) break;
                last_timestamp = t;  // several may lie in the right stride; the last one is always skipped
            }
        double cur_max = 0.0, prev_len = 0.0, penultimate = 0.0;
        int seg_begin = 0;  // current_tokens = the text ids of row[seg_begin .. i)
        for (int i = 0; i < n; ++i) {
            const int t = row[1 + i];
            if (t < tb) continue;  // text (gathered at the close) or an ignored special
            const double ts = __dmul_rn((double)(t - tb), tp);
            if (ts < cur_max) {  // the next segment of a long-form generate has started
                const bool single = i >= 2 && !(row[i] >= tb && row[i - 1] >= tb);
                if (single) {
                    prev_len = __dadd_rn(prev_len, __dmul_rn(tp, (double)a.segment_size));
                } else {
                    cur_max = penultimate;
                    prev_len = __dadd_rn(prev_len, penultimate);
                }
            }
            penultimate = cur_max;
            cur_max = ts;
            const double time = py_round2(__dadd_rn(__dadd_rn(ts, time_offset), prev_len));
            if (last_timestamp >= 0 && t >= last_timestamp) {
                skip = true;  // inside the right stride: resolved by the next chunk, and its pair goes too
            } else if (skip || (n_ops > 0 && (double)t < first_timestamp)) {
                skip = false;
            } else if (!have_start) {
                start = time;
                have_start = true;
            } else if (time == start) {
                // a duplicate of the start: stays a start
            } else {
                operand(strip(row, seg_begin, i), k, time_offset);  // current_tokens is an operand even when it is empty
                flush(time);
                seg_begin = i + 1;
            }
        }
        const double off = time_offset;
        time_offset = __dadd_rn(time_offset, right_start);
        const int R = strip(row, seg_begin, n);
        if (R > 0) {
            operand(R, k, off);
        } else if (!any_ids) {  // nothing pending at all: the open segment's start is forgotten
            n_ops = 0;
            L = 0;
            have_start = false;
        }
    }
    if (n_ops > 0) flush(nan);  // no ending timestamp: end = None
    if (tid == 0) {
        a.merged_len[rec] = min(total, cap);
        a.n_seg[rec] = nseg;
    }
}

size_t chunk_segments_lds_bytes(int stride) { return (size_t)4 * stride * sizeof(int); }

int launch_chunk_segments(const ChunkSegArgs& a, int n_rec, hipStream_t st) {
    if (n_rec <= 0 || a.stride <= 0 || a.cap <= 0 || a.seg_cap <= 0) return launch_refuse("chunk_segments: recordings, ids per row and output capacities must be positive");
    if (a.stride > CHUNK_MERGE_MAX_IDS) return launch_refuse("chunk_segments: more ids per row than the kernel's LDS holds (CHUNK_MERGE_MAX_IDS = 2048)");
    if (a.timestamp_begin < a.first_special || !(a.time_precision > 0.0) || a.segment_size <= 0 || a.tab_cols < a.tab_c0 + 3)
        return launch_refuse("chunk_segments: timestamp_begin below first_special, or a non-positive time_precision / segment_size");
    hipLaunchKernelGGL(chunk_segments_kernel, dim3(n_rec), dim3(CM_THREADS), chunk_segments_lds_bytes(a.stride), st, a);
    return hipGetLastError() == hipSuccess ? WM_LAUNCH_OK : WM_LAUNCH_HIP;
}


}  // namespace wm
