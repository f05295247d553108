// wm_chunked.cpp — chunked long-form transcription: the chunk table, the batched passes and the chunk hooks.
#include "wm_runtime.h"

// ---- chunked long-form transcription -----------------------------------------------------------------------------
// HF's ASR pipeline with chunk_length_s / stride_length_s: overlapping chunks cut by pipelines/automatic_speech_recognition.py::chunk_iter,
// every chunk decoded on its own in batches, the id lists stitched by tokenization_whisper._find_longest_common_sequence.
static const int CHUNK_COLS = 6;  // (recording, start, len, stride_left, stride_right, is_last)
extern "C" int wm_chunk_table(const int32_t* n_samples, int R, int chunk_len, int stride_left, int stride_right, int window, int32_t* table, int cap,
                              int32_t* n_chunks) {
    if (!n_samples || R <= 0 || !n_chunks || cap < 0 || (cap > 0 && !table)) return fail(WM_E_ARG, "bad argument");
    if (chunk_len <= 0 || stride_left < 0 || stride_right < 0) return fail(WM_E_ARG, "chunk_len must be positive and the strides non-negative");
    const int64_t step = (int64_t)chunk_len - stride_left - stride_right;
    if (step <= 0)  // HF: "Chunk length must be superior to stride length" for <; the equal case dies in chunk_iter's range(0, n, 0)
        return fail(WM_E_ARG, "chunk_len %d must exceed stride_left %d + stride_right %d", chunk_len, stride_left, stride_right);
    if (window > 0 && chunk_len > window) return fail(WM_E_ARG, "chunk_len %d exceeds the model's window of %d samples", chunk_len, window);
    int64_t n = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t T = n_samples[r];
        if (T < 0) return fail(WM_E_ARG, "n_samples[%d] = %d is negative", r, n_samples[r]);
        for (int64_t start = 0; start < T; start += step) {
            const int64_t end = start + chunk_len, len = std::min(T, end) - start;
            const int sl = start == 0 ? 0 : stride_left;
            const bool last = end >= T;
            if (len > sl) {
                if (n < cap) {
                    int32_t* t = table + n * CHUNK_COLS;
                    t[0] = r, t[1] = (int32_t)start, t[2] = (int32_t)len, t[3] = sl, t[4] = last ? 0 : stride_right, t[5] = last;
                }
                ++n;
            }
            if (last) break;
        }
    }
    if (n > INT32_MAX) return fail(WM_E_SIZE, "more than 2^31 chunks");
    *n_chunks = (int32_t)n;
    if (table && n > cap) return fail(WM_E_SIZE, "the table holds %d chunks, %lld are needed", cap, (long long)n);
    return 0;
}

extern "C" int wm_op_chunk_gather(float* out, const float* pcm, int R, int64_t T_max, const int32_t* items, int n, int N) {
    if (!out || !pcm || !items || R <= 0 || T_max <= 0 || n <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    for (int k = 0; k < n; ++k) {
        const int32_t* t = items + 3 * (size_t)k;
        if (t[0] < 0 || t[0] >= R || t[1] < 0 || t[2] < 0 || t[2] > N || (int64_t)t[1] + t[2] > T_max)
            return fail(WM_E_ARG, "item %d = (%d, %d, %d) leaves pcm [%d][%lld] or the row of %d samples", k, t[0], t[1], t[2], R, (long long)T_max, N);
    }
    TmpDev tmp;
    DevBuf &dp = tmp.add(), &di = tmp.add(), &dout = tmp.add();
    WMCHK(upload_bytes(dp, pcm, (size_t)R * T_max * 4));
    WMCHK(upload_bytes(di, items, (size_t)n * 3 * 4));
    WMCHK(upload_bytes(dout, out, (size_t)n * N * 4));  // in and out: a store the kernel misses keeps the caller's value
    launch_chunk_gather(dp.as<float>(), di.as<int>(), 3, 0, dout.as<float>(), n, (size_t)T_max, N, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ids [n_rows][stride] + lens [n_rows] -> the packed rows the kernel reads, [n_rows][1 + stride]
extern "C" int wm_op_chunk_merge(int32_t* merged, int32_t* merged_len, const int32_t* ids, const int32_t* lens, const int32_t* rec_off, int n_rows,
                                 int n_rec, int stride, int cap, int first_special) {
    if (!merged || !merged_len || !ids || !lens || !rec_off || n_rows <= 0 || n_rec <= 0 || stride <= 0 || cap <= 0) return fail(WM_E_ARG, "bad argument");
    if (rec_off[0] < 0 || rec_off[n_rec] > n_rows) return fail(WM_E_ARG, "rec_off leaves the %d rows", n_rows);
    for (int r = 0; r < n_rec; ++r)
        if (rec_off[r + 1] < rec_off[r]) return fail(WM_E_ARG, "rec_off must not decrease");
    std::vector<int32_t> packed((size_t)n_rows * (1 + stride), 0);
    for (int k = 0; k < n_rows; ++k) {
        if (lens[k] < 0 || lens[k] > stride) return fail(WM_E_ARG, "lens[%d] = %d outside [0, %d]", k, lens[k], stride);
        packed[(size_t)k * (1 + stride)] = lens[k];
        std::copy(ids + (size_t)k * stride, ids + (size_t)k * stride + lens[k], packed.begin() + (size_t)k * (1 + stride) + 1);
    }
    for (int r = 0; r < n_rec; ++r) {  // cap must hold the recording's ids even when nothing overlaps
        int64_t sum = 0;
        for (int k = rec_off[r]; k < rec_off[r + 1]; ++k) sum += lens[k];
        if (sum > cap) return fail(WM_E_ARG, "recording %d has %lld ids, cap is %d", r, (long long)sum, cap);
    }
    TmpDev tmp;
    DevBuf &dr = tmp.add(), &doff = tmp.add(), &dm = tmp.add(), &dl = tmp.add();
    WMCHK(upload_bytes(dr, packed.data(), packed.size() * 4));
    WMCHK(upload_bytes(doff, rec_off, (size_t)(n_rec + 1) * 4));
    WMCHK(upload_bytes(dm, merged, (size_t)n_rec * cap * 4));  // in and out, as wm_op_chunk_gather
    WMCHK(dl.alloc((size_t)n_rec * 4));
    LCHK(launch_chunk_merge(dr.as<int>(), doff.as<int>(), n_rec, stride, first_special, dm.as<int>(), dl.as<int>(), cap, nullptr));
    HIPCHK(hipMemcpy(merged, dm.p, (size_t)n_rec * cap * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(merged_len, dl.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Chunks of all recordings fill passes of up to max_batch rows, in table order; passes alternate over the caller's slots 0..1 (0..3 under
// coalesce = 2, where two submits make one pass), so two passes are in flight, each with a log-mel buffer of its own.  A pass's ids go
// from its decode state into the packed table on the device (wm_transcribe_wait_device's rows); the stitch reads that table.
// The timestamp outputs of wm_transcribe_chunked_ts.  mode 0: none of this — wm_transcribe_chunked, which launches what it
// always launched.  mode 1 (segments): chunk_segments_kernel stitches instead of chunk_merge_kernel.  mode 2 (word): every pass also
// carries the alignment-head capture with per-row n_frames = len // 160, and its times are packed next to its ids.
struct ChunkTs {
    int mode = 0;
    double time_precision = 0.0;
    int32_t* n_seg = nullptr;
    double* seg_times = nullptr;
    int32_t* seg_range = nullptr;
    int seg_cap = 0;
    double* pairs = nullptr;
    float* chunk_times = nullptr;
};
static int chunked_impl(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                        int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang, int first_special,
                        int32_t* merged, int32_t* merged_len, int cap, int32_t* chunk_ids, int32_t* chunk_n, int32_t* n_passes, const ChunkTs& ts) {
    if (!m || !pcm || !n_samples || R <= 0 || stride <= 0 || !merged || !merged_len || cap <= 0 || (!chunk_ids != !chunk_n) || first_special <= 0)
        return fail(WM_E_ARG, "bad argument");
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    WMCHK(check_opts(m, o, 1));
    if (m->top_k > 0)  // (the stitched result has no place for them yet)
        return fail(WM_E_ARG, "top-k alternatives (wm_set_top_k) are not available in chunked transcription: set top_k to 0");
    if (m->repeat.ct)  // (the window and chunk schedulers do not carry the rows' trie nodes yet)
        return fail(WM_E_ARG, "the phrase-list constraint (wm_set_constraint) is not available in chunked transcription: clear it first");
    const bool word = ts.mode == 2;
    if (ts.mode) {  // everything is refused before anything is launched
        if (ts.mode != 1 && ts.mode != 2) return fail(WM_E_ARG, "mode must be 1 (segments) or 2 (word)");
        if (!ts.n_seg || !ts.seg_times || !ts.seg_range || ts.seg_cap <= 0 || (word && !ts.pairs) || (ts.chunk_times && (!word || !chunk_ids)))
            return fail(WM_E_ARG, "bad argument");
        if (o->timestamp_begin <= 0) return fail(WM_E_ARG, "chunked timestamps need the timestamp rule (opts->timestamp_begin)");
        if (o->timestamp_begin < first_special) return fail(WM_E_ARG, "timestamp_begin %d lies below first_special %d", o->timestamp_begin, first_special);
        if (word && m->align_pairs.empty()) return fail(WM_E_ARG, "word timestamps need alignment heads (wm_set_alignment_heads)");
        if (word && lang_ids) return fail(WM_E_ARG, "word timestamps do not combine with language detection (a language pass carries no token timestamps)");
        if (ts.time_precision < 0.0 || ts.time_precision != ts.time_precision) return fail(WM_E_ARG, "time_precision must be positive (0: the model's)");
    }
    for (int r = 0; r < R; ++r)
        if (n_samples[r] < 0 || n_samples[r] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", r, n_samples[r]);
    int32_t n = 0;
    WMCHK(wm_chunk_table(n_samples, R, chunk_len, stride_left, stride_right, N, nullptr, 0, &n));
    std::vector<int32_t> tab((size_t)std::max(n, 1) * CHUNK_COLS), off(R + 1, 0);
    WMCHK(wm_chunk_table(n_samples, R, chunk_len, stride_left, stride_right, N, tab.data(), n, &n));
    for (int k = 0; k < n; ++k) ++off[tab[(size_t)k * CHUNK_COLS] + 1];
    int most = 0;
    for (int r = 0; r < R; ++r) {
        most = std::max(most, off[r + 1]);
        off[r + 1] += off[r];
    }
    const int total = o->n_prompt + 1 + o->max_loop;
    if ((int64_t)most * total > cap) return fail(WM_E_SIZE, "cap %d is smaller than %d chunks x %d ids of the longest recording", cap, most, total);
    if (ts.mode && total > CHUNK_MERGE_MAX_IDS) return fail(WM_E_ARG, "more than %d ids per chunk", CHUNK_MERGE_MAX_IDS);
    if (word)
        for (int k = 0; k < n; ++k)
            if (tab[(size_t)k * CHUNK_COLS + 2] < 2 * FE_HOP)
                return fail(WM_E_ARG, "chunk %d has %d samples: word timestamps need two mel frames of audio per chunk", k, tab[(size_t)k * CHUNK_COLS + 2]);
    if (ts.mode) std::fill(ts.n_seg, ts.n_seg + R, 0);
    const int PB = std::min(m->cfg.max_batch, std::max(n, 1));
    if (lang_ids) {  // what a _lang pass would refuse, before anything is launched
        WMCHK(lang_list_check(c.vocab, lang_ids, n_lang));
        if (o->n_prompt < 2) return fail(WM_E_ARG, "language detection needs at least two initial ids");
        if (dec_lanes_for(PB) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    }
    if (n_passes) *n_passes = 0;
    std::fill(merged_len, merged_len + R, 0);
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    WMCHK(flush_held(m));
    const int NS = m->cfg.coalesce == 2 ? 4 : 2;
    for (int s = 0; s < NS; ++s)
        if (m->slot_ref[s].pending) return fail(WM_E_STATE, "slot %d still holds a pass that was not waited for (chunked transcription uses slots 0..%d)", s, NS - 1);
    hipStream_t st = m->stream;
    TmpDev tmp;
    DevBuf &d_pcm = tmp.add(), &d_tab = tmp.add(), &d_off = tmp.add(), &d_packed = tmp.add(), &d_merged = tmp.add(), &d_len = tmp.add();
    DevBuf &d_times = tmp.add(), &d_nseg = tmp.add(), &d_segt = tmp.add(), &d_segr = tmp.add(), &d_pairs = tmp.add();
    if (ts.mode) {
        WMCHK(d_nseg.alloc((size_t)R * 4));
        WMCHK(d_segt.alloc((size_t)R * ts.seg_cap * 2 * 8));
        WMCHK(d_segr.alloc((size_t)R * ts.seg_cap * 2 * 4));
    }
    if (word) {
        WMCHK(d_times.alloc((size_t)n * total * 4));
        WMCHK(d_pairs.alloc((size_t)R * cap * 2 * 8));
    }
    const float* dpcm = pcm;
    if (!pcm_on_device) {
        WMCHK(d_pcm.alloc((size_t)R * stride * 4));
        HIPCHK(hipMemcpyAsync(d_pcm.p, pcm, (size_t)R * stride * 4, hipMemcpyHostToDevice, st));
        dpcm = d_pcm.as<float>();
    }
    WMCHK(d_tab.alloc(tab.size() * 4));
    WMCHK(d_off.alloc(off.size() * 4));
    WMCHK(d_packed.alloc((size_t)n * (1 + total) * 4));
    WMCHK(d_merged.alloc((size_t)R * cap * 4));
    WMCHK(d_len.alloc((size_t)R * 4));
    HIPCHK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));  // the chunk table and (below) its recording offsets: all that crosses the bus
    HIPCHK(hipMemcpyAsync(d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    DevBuf* d_mel[4];
    for (int s = 0; s < NS; ++s) {
        d_mel[s] = &tmp.add();
        WMCHK(d_mel[s]->alloc((size_t)PB * c.n_mels * n_frames * 4));
    }
    struct Pend {
        int row0 = 0, rows = 0;
        bool live = false;
    } pend[4];
    auto collect = [&](int s) {
        Pend& p = pend[s];
        p.live = false;
        PassOut out;
        out.dev_packed = d_packed.as<int32_t>() + (size_t)p.row0 * (1 + total);
        out.rows_cap = p.rows;
        out.pack_stride = total;
        if (word) out.dev_times = d_times.as<float>() + (size_t)p.row0 * total;  // this pass's times, next to its ids
        return collect_slot(m, s, PassKind::transcribe, out);
    };
    int rc = 0, np = 0;
    std::string err;
    for (int row0 = 0; row0 < n && !rc; row0 += PB, ++np) {
        const int s = np % NS, rows = std::min(PB, n - row0);
        if (pend[s].live) rc = collect(s);
        if (!rc) {
            launch_chunk_gather(dpcm, d_tab.as<int>(), CHUNK_COLS, row0, m->fe.pcm.as<float>(), rows, (size_t)stride, N, st);
            rc = frontend_compute(m, rows, d_mel[s]->as<float>());
        }
        if (!rc && word) {  // the ragged form of §28: row b keeps (len // 160) // 2 encoder positions
            std::vector<int32_t> nf(rows), cols;
            for (int b = 0; b < rows; ++b) nf[b] = tab[(size_t)(row0 + b) * CHUNK_COLS + 2] / FE_HOP;
            rc = align_cols(m, nf.data(), rows, cols);
            if (!rc) {
                PassAsk ask{d_mel[s]->as<float>(), 1, rows, o};
                ask.cols = &cols;
                rc = submit_slot(m, s, ask);
            }
        } else if (!rc)
            rc = lang_ids ? lang_entry(m, s, d_mel[s]->as<float>(), 1, rows, o, nullptr, nullptr, 0, false, -1, o->n_prompt, lang_ids, n_lang, PassOut())
                          : submit_slot(m, s, PassAsk{d_mel[s]->as<float>(), 1, rows, o});
        if (!rc) {
            pend[s].row0 = row0, pend[s].rows = rows, pend[s].live = true;
        } else {
            err = g_err;
        }
    }
    for (int k = 0; k < NS; ++k) {  // the oldest pass first; after a failure the rest is still collected, so no slot stays pending
        const int s = (np + k) % NS;
        if (!pend[s].live) continue;
        const int rc2 = collect(s);
        if (rc2 && !rc) rc = rc2, err = g_err;
    }
    if (rc) {
        (void)hipStreamSynchronize(st);  // the scratch is released on return
        g_err = err;
        return rc;
    }
    if (n_passes) *n_passes = np;
    if (ts.mode) {
        ChunkSegArgs a{};
        a.rows = d_packed.as<int>();
        a.rec_off = d_off.as<int>();
        a.tab = d_tab.as<int>();
        a.times = word ? d_times.as<float>() : nullptr;
        a.tab_cols = CHUNK_COLS, a.tab_c0 = 2, a.stride = total, a.first_special = first_special, a.timestamp_begin = o->timestamp_begin;
        a.segment_size = c.n_audio_ctx;
        a.time_precision = ts.time_precision > 0.0 ? ts.time_precision : (double)N / 16000.0 / (double)c.n_audio_ctx;
        a.merged = d_merged.as<int>(), a.merged_len = d_len.as<int>(), a.n_seg = d_nseg.as<int>();
        a.seg_times = (double*)d_segt.p, a.seg_range = d_segr.as<int>(), a.pairs = word ? (double*)d_pairs.p : nullptr;
        a.cap = cap, a.seg_cap = ts.seg_cap;
        LCHK(launch_chunk_segments(a, R, st));
        HIPCHK(hipMemcpyAsync(ts.n_seg, d_nseg.p, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    } else {
        LCHK(launch_chunk_merge(d_packed.as<int>(), d_off.as<int>(), R, total, first_special, d_merged.as<int>(), d_len.as<int>(), cap, st));
    }
    HIPCHK(hipMemcpyAsync(merged_len, d_len.p, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < R && ts.mode; ++r)
        if (ts.n_seg[r] > ts.seg_cap) return fail(WM_E_SIZE, "recording %d has %d segments, seg_cap is %d", r, ts.n_seg[r], ts.seg_cap);
    for (int r = 0; r < R; ++r) {
        if (merged_len[r] > 0)
            HIPCHK(hipMemcpyAsync(merged + (size_t)r * cap, d_merged.as<int32_t>() + (size_t)r * cap, (size_t)merged_len[r] * 4, hipMemcpyDeviceToHost, st));
        if (word && merged_len[r] > 0)
            HIPCHK(hipMemcpyAsync(ts.pairs + (size_t)r * cap * 2, (const double*)d_pairs.p + (size_t)r * cap * 2, (size_t)merged_len[r] * 16, hipMemcpyDeviceToHost, st));
        if (ts.mode && ts.n_seg[r] > 0) {
            const size_t at = (size_t)r * ts.seg_cap * 2;
            HIPCHK(hipMemcpyAsync(ts.seg_times + at, (const double*)d_segt.p + at, (size_t)ts.n_seg[r] * 16, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(ts.seg_range + at, d_segr.as<int32_t>() + at, (size_t)ts.n_seg[r] * 8, hipMemcpyDeviceToHost, st));
        }
    }
    if (ts.chunk_times)
        HIPCHK(hipMemcpyAsync(ts.chunk_times, d_times.p, (size_t)n * total * 4, hipMemcpyDeviceToHost, st));
    if (chunk_ids) {  // on request: every chunk's own ids, as wm_transcribe_pcm of that chunk's samples returns them
        HIPCHK(hipMemcpy2DAsync(chunk_n, 4, d_packed.p, (size_t)(1 + total) * 4, 4, n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(chunk_ids, (size_t)total * 4, d_packed.as<int32_t>() + 1, (size_t)(1 + total) * 4, (size_t)total * 4, n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int wm_transcribe_chunked(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                                     int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang, int first_special,
                                     int32_t* merged, int32_t* merged_len, int cap, int32_t* chunk_ids, int32_t* chunk_n, int32_t* n_passes) {
    return chunked_impl(m, pcm, pcm_on_device, n_samples, R, stride, chunk_len, stride_left, stride_right, o, lang_ids, n_lang, first_special, merged,
                        merged_len, cap, chunk_ids, chunk_n, n_passes, ChunkTs());
}
extern "C" int wm_transcribe_chunked_ts(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                                        int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang,
                                        int first_special, int mode, double time_precision, int32_t* merged, int32_t* merged_len, int cap,
                                        int32_t* n_seg, double* seg_times, int32_t* seg_range, int seg_cap, double* pairs, int32_t* chunk_ids,
                                        int32_t* chunk_n, float* chunk_times, int32_t* n_passes) {
    ChunkTs ts;
    ts.mode = mode;
    ts.time_precision = time_precision;
    ts.n_seg = n_seg, ts.seg_times = seg_times, ts.seg_range = seg_range, ts.seg_cap = seg_cap, ts.pairs = pairs, ts.chunk_times = chunk_times;
    if (mode != 1 && mode != 2) return fail(WM_E_ARG, "mode must be 1 (segments) or 2 (word)");
    return chunked_impl(m, pcm, pcm_on_device, n_samples, R, stride, chunk_len, stride_left, stride_right, o, lang_ids, n_lang, first_special, merged,
                        merged_len, cap, chunk_ids, chunk_n, n_passes, ts);
}

// chunk_segments_kernel alone: ids [n_rows][stride] with lens [n_rows], strides [n_rows][3] = (len, stride_left, stride_right) in samples,
// times [n_rows][stride] (word mode) or NULL (segments mode).  The outputs are uploaded first, so a cell the kernel does not store
// keeps the caller's value.
extern "C" int wm_op_chunk_segments(const int32_t* ids, const int32_t* lens, const int32_t* strides, const float* times, const int32_t* rec_off,
                                    int n_rows, int n_rec, int stride, int first_special, int timestamp_begin, double time_precision,
                                    int segment_size, int32_t* merged, int32_t* merged_len, int cap, int32_t* n_seg, double* seg_times,
                                    int32_t* seg_range, int seg_cap, double* pairs) {
    if (!ids || !lens || !strides || !rec_off || !merged || !merged_len || !n_seg || !seg_times || !seg_range || n_rows <= 0 || n_rec <= 0 ||
        stride <= 0 || cap <= 0 || seg_cap <= 0 || (times && !pairs))
        return fail(WM_E_ARG, "bad argument");
    if (rec_off[0] < 0 || rec_off[n_rec] > n_rows) return fail(WM_E_ARG, "rec_off leaves the %d rows", n_rows);
    for (int r = 0; r < n_rec; ++r)
        if (rec_off[r + 1] < rec_off[r]) return fail(WM_E_ARG, "rec_off must not decrease");
    std::vector<int32_t> packed((size_t)n_rows * (1 + stride), 0);
    for (int k = 0; k < n_rows; ++k) {
        if (lens[k] < 0 || lens[k] > stride) return fail(WM_E_ARG, "lens[%d] = %d outside [0, %d]", k, lens[k], stride);
        if (strides[3 * k] < 0 || strides[3 * k + 1] < 0 || strides[3 * k + 2] < 0) return fail(WM_E_ARG, "strides[%d] is negative", k);
        packed[(size_t)k * (1 + stride)] = lens[k];
        std::copy(ids + (size_t)k * stride, ids + (size_t)k * stride + lens[k], packed.begin() + (size_t)k * (1 + stride) + 1);
    }
    for (int r = 0; r < n_rec; ++r) {  // cap must hold the recording's ids even when nothing overlaps
        int64_t sum = 0;
        for (int k = rec_off[r]; k < rec_off[r + 1]; ++k) sum += lens[k];
        if (sum > cap) return fail(WM_E_SIZE, "recording %d has %lld ids, cap is %d", r, (long long)sum, cap);
    }
    TmpDev tmp;
    DevBuf &dr = tmp.add(), &doff = tmp.add(), &dtab = tmp.add(), &dtt = tmp.add(), &dm = tmp.add(), &dl = tmp.add(), &dn = tmp.add(), &dst = tmp.add(),
           &dsr = tmp.add(), &dp = tmp.add();
    const size_t nm = (size_t)n_rec * cap, ns = (size_t)n_rec * seg_cap * 2;
    WMCHK(upload_bytes(dr, packed.data(), packed.size() * 4));
    WMCHK(upload_bytes(doff, rec_off, (size_t)(n_rec + 1) * 4));
    WMCHK(upload_bytes(dtab, strides, (size_t)n_rows * 3 * 4));
    WMCHK(upload_bytes(dm, merged, nm * 4));
    WMCHK(dl.alloc((size_t)n_rec * 4));
    WMCHK(dn.alloc((size_t)n_rec * 4));
    WMCHK(upload_bytes(dst, seg_times, ns * 8));
    WMCHK(upload_bytes(dsr, seg_range, ns * 4));
    if (times) {
        WMCHK(upload_bytes(dtt, times, (size_t)n_rows * stride * 4));
        WMCHK(upload_bytes(dp, pairs, nm * 2 * 8));
    }
    ChunkSegArgs a{};
    a.rows = dr.as<int>(), a.rec_off = doff.as<int>(), a.tab = dtab.as<int>(), a.times = times ? dtt.as<float>() : nullptr;
    a.tab_cols = 3, a.tab_c0 = 0, a.stride = stride, a.first_special = first_special, a.timestamp_begin = timestamp_begin;
    a.segment_size = segment_size, a.time_precision = time_precision;
    a.merged = dm.as<int>(), a.merged_len = dl.as<int>(), a.n_seg = dn.as<int>(), a.seg_times = (double*)dst.p, a.seg_range = dsr.as<int>();
    a.pairs = times ? (double*)dp.p : nullptr;
    a.cap = cap, a.seg_cap = seg_cap;
    LCHK(launch_chunk_segments(a, n_rec, nullptr));
    HIPCHK(hipMemcpy(merged, dm.p, nm * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(merged_len, dl.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_seg, dn.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(seg_times, dst.p, ns * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(seg_range, dsr.p, ns * 4, hipMemcpyDeviceToHost));
    if (times) HIPCHK(hipMemcpy(pairs, dp.p, nm * 2 * 8, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_rec; ++r)
        if (n_seg[r] > seg_cap) return fail(WM_E_SIZE, "recording %d has %d segments, seg_cap is %d", r, n_seg[r], seg_cap);
    return 0;
}
