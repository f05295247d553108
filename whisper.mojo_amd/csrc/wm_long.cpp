// wm_long.cpp — sequential long-form transcription: segments, prompts, the window scheduler, the long entries and
// the result getters.
#include "wm_runtime.h"

// ---- sequential long-form transcription (thresholds and no-speech window skipping: §18) -----------------------------
struct wm_long_result {
    std::vector<std::vector<int32_t>> tokens;  // per utterance: the concatenation of its segments' ids
    std::vector<std::vector<wm_segment>> segs;
    int windows = 0, stalled = 0, passes = 0, rows = 0;
    int longest_prompt = 0, row_passes = 0;  // longest decoder prompt a window of a real utterance carried; passes that went per row
    // thresholds (quality = either use_* flag of wm_long_opts was set): per utterance the window log in decode order,
    // skipped windows included, and each segment's window values
    struct Window {
        int64_t seek;
        float avg_logprob, no_speech_prob;
        int32_t skipped;
    };
    bool quality = false;
    int skipped = 0;
    std::vector<std::vector<Window>> wins;
    std::vector<std::vector<float>> seg_avg, seg_nsp;
    // token timestamps (tt = the run computed them): per utterance one time per id of `tokens`
    bool tt = false;
    std::vector<std::vector<double>> times;
};

// The times of one window's kept ids: win[i] is generated id i's time with the window's offset (what align_window_kernel wrote);
// each segment takes its own slice, so the trailing eot and the ids behind the last kept segment leave no entry.
static void long_slice_times(const double* win, const std::vector<wm_segment>& segs, std::vector<double>& out) {
    for (const wm_segment& sg : segs) out.insert(out.end(), win + sg.first, win + sg.first + sg.count);
}
// align_window_kernel's arithmetic on the host, for wm_op_long_token_times: window-relative fp32 times -> float64 with time_offset
static void long_window_times(const float* rel, int n, int64_t seek, std::vector<double>& win) {
#pragma clang fp contract(off)
    const double off = (double)seek * 0.02 / 2;
    win.resize(n);
    for (int i = 0; i < n; ++i) win[i] = (double)rel[i] + off;
}

// HF WhisperGenerationMixin._retrieve_segment (time_precision 0.02, time_precision_features 0.01, input_stride 2) on one window's
// generated ids without the trailing eot.  Returns the seek advance in frames exactly as HF computes it (possibly 0).
static int long_segments(const int32_t* ids, int n, int tb, int64_t seek, int snf, std::vector<wm_segment>& out) {
#pragma clang fp contract(off)
    out.clear();
    const double off = (double)seek * 0.02 / 2;  // time_offset: float64(seek) * time_precision / input_stride
    auto ts = [&](int i) { return ids[i] >= tb; };
    const bool single_end = n >= 2 && !ts(n - 2) && ts(n - 1);  // timestamp_tokens[-2:] == [False, True]
    std::vector<int> slices;
    for (int i = 1; i < n; ++i)
        if (ts(i - 1) && ts(i)) slices.push_back(i);  // consecutive timestamps end a segment
    if (!slices.empty()) {
        if (single_end) slices.push_back(n);
        else slices.back() += 1;  // the last pair stays in the last segment
        int last = 0;
        for (size_t k = 0; k < slices.size(); ++k) {
            const int cur = slices[k];
            const bool is_last = k + 1 == slices.size();
            const int end_i = (!is_last || single_end) ? cur - 1 : cur - 2;
            out.push_back(wm_segment{last, cur - last, off + (double)(ids[last] - tb) * 0.02, off + (double)(ids[end_i] - tb) * 0.02});
            last = cur;
        }
        return single_end ? snf : (ids[last - 2] - tb) * 2;
    }
    // no pair: the whole window is one segment, ending at the last timestamp (other than <|0.00|>) or at the window's end — the
    // latter as HF computes it, int(seek_num_frames * 0.01 / 0.02) in float32 (a long tensor times a Python float)
    int last_ts = -1;
    for (int i = 0; i < n; ++i)
        if (ts(i)) last_ts = ids[i];
    const double end_pos = (last_ts >= 0 && last_ts != tb) ? (double)(last_ts - tb) : (double)(int)((float)snf * 0.01f / 0.02f);
    out.push_back(wm_segment{0, n, off, off + end_pos * 0.02});
    return snf;
}

extern "C" int wm_op_long_segments(const int32_t* ids, int n, int timestamp_begin, int64_t seek, int seek_num_frames, wm_segment* segs,
                                   int32_t* n_segs, int32_t* advance) {
    if (n < 0 || (n > 0 && !ids) || !segs || !n_segs || !advance || timestamp_begin <= 0 || seek < 0 || seek_num_frames < 0)
        return fail(WM_E_ARG, "bad argument");
    std::vector<wm_segment> out;
    *advance = long_segments(ids, n, timestamp_begin, seek, seek_num_frames, out);
    *n_segs = (int32_t)out.size();
    std::copy(out.begin(), out.end(), segs);
    return 0;
}

// The long-form scratch that grows with the audio goes back to the device once a call is done (the two decode states stay, like the
// slots').  hipFree waits for the device, and every pass of the call has been waited for.
void long_release(wm_model* m) {
    wm_model::LongForm& L = m->lf;
    DevBuf* bs[] = {&L.pcm, &L.lens, &L.frames, &L.spec, &L.part, &L.mel, &L.in_mel, &L.win[0], &L.win[1], &L.items[0], &L.items[1]};
    for (DevBuf* b : bs) b->release();
}

// HF WhisperGenerationMixin._prepare_decoder_input_ids for ONE utterance (wm_op_long_prompt).  seq / segs: the utterance's segments
// so far; the first-segment pseudo-segment (prompt_ids minus a leading <|startofprev|>) is entered in front of them here.
static bool long_opts_plain(const wm_long_opts* lo) { return !lo || (!lo->condition_on_prev_tokens && (!lo->prompt_ids || lo->n_prompt_ids <= 0)); }
static void long_prompt(const int32_t* seq, const wm_segment* segs, int n_segs, const int32_t* init, int n_init, const wm_long_opts* lo, int tb,
                        int n_text_ctx, std::vector<int32_t>& out) {
    out.clear();
    const bool have_prompt = lo && lo->prompt_ids && lo->n_prompt_ids > 0;
    const bool cond = lo && lo->condition_on_prev_tokens;
    const bool all_segments = lo && lo->prompt_condition_type == 1;
    const int pseudo0 = have_prompt && lo->prompt_ids[0] == lo->prev_sot_token ? 1 : 0;
    const bool pseudo = have_prompt && !all_segments;
    if (cond && (n_segs > 0 || pseudo)) {
        const int cut = n_text_ctx / 2 - 1;
        std::vector<int32_t> prev;
        auto add = [&](const int32_t* t, int n) {  // skip_ending_double_timestamps
            if (n > 2 && t[n - 2] >= tb) --n;
            prev.insert(prev.end(), t, t + n);
        };
        if (pseudo) add(lo->prompt_ids + pseudo0, lo->n_prompt_ids - pseudo0);
        for (int i = 0; i < n_segs; ++i) add(seq + segs[i].first, segs[i].count);
        if ((int)prev.size() > cut) prev.erase(prev.begin(), prev.end() - cut);
        if (have_prompt && all_segments)
            out.assign(lo->prompt_ids, lo->prompt_ids + lo->n_prompt_ids);
        else
            out.push_back(lo->prev_sot_token);
        out.insert(out.end(), prev.begin(), prev.end());
    } else if (have_prompt) {
        out.assign(lo->prompt_ids, lo->prompt_ids + lo->n_prompt_ids);
    }
    out.insert(out.end(), init, init + n_init);
}
static int long_opts_check(const wm_long_opts* lo, const int32_t* init, int n_init, int max_loop, int vocab, int n_text_ctx, int pass_rows) {
    if (lo && lo->use_no_speech_threshold) {  // HF dereferences logprob_threshold whenever no_speech_threshold is set
        if (!lo->use_logprob_threshold) return fail(WM_E_ARG, "no_speech_threshold needs logprob_threshold");
        if (lo->no_speech_token < 0 || lo->no_speech_token >= vocab) return fail(WM_E_ARG, "no_speech_token %d is not a vocabulary id", lo->no_speech_token);
    }
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold) && lo->no_speech_token != -1 &&
        (lo->no_speech_token < 0 || lo->no_speech_token >= vocab))  // (-1 with logprob_threshold alone: no probe, no_speech_prob is NaN)
        return fail(WM_E_ARG, "no_speech_token %d is neither -1 nor a vocabulary id", lo->no_speech_token);
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold) && dec_lanes_for(pass_rows) != 1)
        return fail(WM_E_ARG, "log-probabilities need a single-lane decode state");
    if (long_opts_plain(lo)) {
        if (lo && lo->prompt_condition_type == 1) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
        return 0;
    }
    (void)init;
    if (dec_lanes_for(pass_rows) != 1) return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    const int cut = n_text_ctx / 2 - 1;
    const int np = lo->prompt_ids ? std::max(lo->n_prompt_ids, 0) : 0;
    if (lo->n_prompt_ids < 0 || (lo->n_prompt_ids > 0 && !lo->prompt_ids)) return fail(WM_E_ARG, "bad prompt_ids");
    if (lo->prompt_condition_type != 0 && lo->prompt_condition_type != 1) return fail(WM_E_ARG, "prompt_condition_type must be 0 (first-segment) or 1 (all-segments)");
    if (lo->prompt_condition_type == 1 && !lo->condition_on_prev_tokens) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
    if (lo->prev_sot_token < 0 || lo->prev_sot_token >= vocab) return fail(WM_E_ARG, "prev_sot_token %d is not a vocabulary id", lo->prev_sot_token);
    for (int i = 0; i < np; ++i)
        if (lo->prompt_ids[i] < 0 || lo->prompt_ids[i] >= vocab) return fail(WM_E_ARG, "prompt id out of range");
    if (np > cut + 1) return fail(WM_E_ARG, "n_prompt_ids %d exceeds %d (half the decoder context)", np, cut + 1);
    const int worst = lo->condition_on_prev_tokens ? ((lo->prompt_condition_type == 1 && np > 0 ? np : 1) + cut + n_init) : np + n_init;
    if (worst + 1 + max_loop > n_text_ctx)
        return fail(WM_E_ARG, "longest decoder prompt %d + 1 + max_loop %d exceeds the decoder context %d", worst, max_loop, n_text_ctx);
    return 0;
}
extern "C" int wm_op_long_prompt(const int32_t* seq, const wm_segment* segs, int n_segs, const int32_t* init, int n_init, const wm_long_opts* lo,
                                 int timestamp_begin, int n_text_ctx, int32_t* out, int32_t* n_out) {
    if (n_segs < 0 || (n_segs > 0 && (!seq || !segs)) || !init || n_init <= 0 || !out || !n_out || n_text_ctx < 4 || timestamp_begin <= 0)
        return fail(WM_E_ARG, "bad argument");
    if (lo) {
        if (lo->n_prompt_ids < 0 || (lo->n_prompt_ids > 0 && !lo->prompt_ids)) return fail(WM_E_ARG, "bad prompt_ids");
        if (lo->prompt_condition_type != 0 && lo->prompt_condition_type != 1) return fail(WM_E_ARG, "prompt_condition_type must be 0 (first-segment) or 1 (all-segments)");
        if (lo->prompt_condition_type == 1 && !lo->condition_on_prev_tokens) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
        if (!long_opts_plain(lo) && lo->prev_sot_token < 0) return fail(WM_E_ARG, "prev_sot_token is required with conditioning or prompt_ids");
        if (lo->prompt_ids && lo->n_prompt_ids > n_text_ctx / 2) return fail(WM_E_ARG, "n_prompt_ids %d exceeds %d (half the decoder context)", lo->n_prompt_ids, n_text_ctx / 2);
    }
    for (int i = 0; i < n_segs; ++i)
        if (segs[i].first < 0 || segs[i].count < 0) return fail(WM_E_ARG, "bad segment %d", i);
    std::vector<int32_t> v;
    long_prompt(seq, segs, n_segs, init, n_init, lo, timestamp_begin, n_text_ctx, v);
    if ((int)v.size() > n_text_ctx) return fail(WM_E_ARG, "the prompt (%d ids) exceeds the decoder context %d", (int)v.size(), n_text_ctx);
    std::copy(v.begin(), v.end(), out);
    *n_out = (int32_t)v.size();
    return 0;
}

static int long_check(wm_model* m, const wm_decode_opts* o, int B) {
    WMCHK(check_opts(m, o, B));
    if (o->timestamp_begin <= 0) return fail(WM_E_ARG, "long-form transcription needs the timestamp rules (timestamp_begin > 0)");
    if (o->ignore_eot) return fail(WM_E_ARG, "long-form transcription stops each window at eot (ignore_eot must be 0)");
    if (o->n_prompt + 1 + o->max_loop > m->cfg.dims.n_text_ctx)
        return fail(WM_E_ARG, "n_prompt + 1 + max_loop = %d exceeds the decoder context %d", o->n_prompt + 1 + o->max_loop, m->cfg.dims.n_text_ctx);
    if (m->held.active) return fail(WM_E_STATE, "a coalesced submit is held: wait for it before long-form transcription");
    return 0;
}

// The window scheduler.  Without condition_on_prev_tokens an utterance carries nothing but seek from one window to the next, so a
// pass may take ANY pending (utterance, seek) items: passes of R = min(ceil(B / 2), max_batch) rows (short passes repeat their first
// item, so neither state is re-created within a call and the repeat finishes with its original), two in flight on m->lf.st[0..1]
// — one pass's gather + encoder and the host's segment bookkeeping overlap the other's decode.  An utterance rides one pass at a
// time: with B <= 2R the two states keep the utterances they started with, and when one state runs dry the other's tail runs
// one pass at a time.  mel: device [B][n_mels][T].
// lo (conditioning / prompt_ids): a row's decoder prompt is built from its utterance's own segments when the row is
// assigned to a pass; a pass whose rows all carry opts->prompt goes out exactly as before, any other as a per-row pass.
// lang_ids != null: HF detects once per recording, on its first window — before the loop every recording's window at
// seek 0 is gathered in groups of R rows and run through wm_detect_language's device path on state 0, the ids are read back once per
// group, and from then on recording b's initial ids are opts->prompt with slot 1 replaced by its language: every pass is a per-row pass.
static int long_run(wm_model* m, const float* mel, int T, const int32_t* nf, int B, const wm_decode_opts* o, wm_long_result* res,
                    const wm_long_opts* lo, const int32_t* lang_ids = nullptr, int n_lang = 0, int32_t* lang_out = nullptr, bool tt = false) {
    const wm_dims& c = m->cfg.dims;
    if (m->top_k > 0)  // (no entry of the long-form result carries them yet)
        return fail(WM_E_ARG, "top-k alternatives (wm_set_top_k) are not available in long-form transcription: set top_k to 0");
    if (m->repeat.ct)  // (the window and chunk schedulers do not carry the rows' trie nodes yet)
        return fail(WM_E_ARG, "the phrase-list constraint (wm_set_constraint) is not available in long-form transcription: clear it first");
    const bool plain = long_opts_plain(lo) && !lang_ids;
    // thresholds: every pass is a log-prob pass; with a no_speech_token it also carries the probe at the first of the
    // o->n_prompt initial ids.  A window is skipped iff avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold.
    const bool quality = lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold);
    const NsAsk ns = quality && lo->no_speech_token >= 0 ? NsAsk{lo->no_speech_token, o->n_prompt} : NsAsk();  // (range checked up front)
    res->quality = quality;
    // half the batch per state (when it fits), so that two passes are in flight whenever two utterances are pending
    const int W = 2 * c.n_audio_ctx, R = std::min((B + 1) / 2, m->cfg.max_batch), total = plain ? o->n_prompt + 1 + o->max_loop : c.n_text_ctx;
    std::vector<int32_t> row_prompts[2], row_len[2];  // per state: the pass's prompts [R][n_text_ctx] and their lengths
    int pass_total[2] = {total, total};
    std::vector<int32_t> pr;
    wm_model::LongForm& L = m->lf;
    std::vector<int64_t> seek(B, 0);
    std::vector<char> busy(B, 0);
    std::vector<int> snf(B, 0);
    int n_items[2] = {0, 0}, order[2] = {0, 0}, ticket = 0;
    for (int k = 0; k < 2; ++k) {
        WMCHK(grow(L.win[k], (size_t)R * c.n_mels * W * 4));
        WMCHK(grow(L.items[k], (size_t)R * 3 * 4));
    }
    std::vector<int32_t> toks((size_t)R * total), cnt(R);
    std::vector<float> lps(quality ? (size_t)R * total : 0), avg(R, 0.f), nsp(R, NAN);
    std::vector<wm_segment> segs;
    PassOut out{toks.data(), cnt.data()};
    out.token_logprobs = quality ? lps.data() : nullptr;
    out.avg_logprob = quality ? avg.data() : nullptr;
    out.no_speech_prob = ns.token >= 0 ? nsp.data() : nullptr;
    // token timestamps: every window pass carries the alignment capture and the chain; per state the columns kept per
    // row (window frames / 2) and the window table the finishing kernel reads, per pass the times [R][max_loop + 1] it hands back
    const int L1 = o->max_loop + 1;
    std::vector<double> wt(tt ? (size_t)R * L1 : 0);
    std::vector<int32_t> win_cols[2];
    WinAsk win_ask[2];
    out.win_times = tt ? wt.data() : nullptr;
    res->tt = tt;
    auto collect = [&](int k) { return wait_on(m, L.st[k], 0, -1, out); };
    auto window_ask = [&](int k, const wm_decode_opts* opts) {  // a pass over state k's gathered windows
        PassAsk ask{L.win[k].as<float>(), 1, R, opts};
        ask.lp = quality;
        ask.ns = ns;
        ask.rp = m->repeat;  // every window's pass sees its own decoder ids only, carried previous text included (HF's per-window generate)
        if (tt) {
            win_cols[k].resize(R);
            for (int r = 0; r < R; ++r) win_cols[k][r] = std::max(1, L.h_items[k][3 * r + 2] / 2);
            win_ask[k] = WinAsk{L.items[k].as<int>(), n_items[k]};
            ask.cols = &win_cols[k];
            ask.win = &win_ask[k];
        }
        return ask;
    };
    auto drain = [&]() {  // an error mid-run: let the other pass finish before returning
        for (int k = 0; k < 2; ++k)
            if (n_items[k] && L.st[k] && L.st[k]->pending) (void)collect(k);
    };
    std::vector<int32_t> inits;  // language detection: [B][n_prompt] each recording's own initial ids
    if (lang_ids) {
        std::vector<int32_t>& h = L.h_items[0];
        for (int b0 = 0; b0 < B; b0 += R) {
            const int nb = std::min(R, B - b0);
            h.clear();
            for (int r = 0; r < R; ++r) {  // (spare rows repeat the group's first recording)
                const int b = b0 + (r < nb ? r : 0);
                h.insert(h.end(), {b, 0, (int32_t)std::min<int64_t>(nf[b], W)});
            }
            HIPCHK(hipMemcpyAsync(L.items[0].p, h.data(), (size_t)R * 3 * 4, hipMemcpyHostToDevice, m->stream));
            launch_window_gather(mel, L.items[0].as<int>(), L.win[0].as<float>(), R, c.n_mels, T, W, m->stream);
            HIPCHK(hipGetLastError());
            WMCHK(submit_on(m, &L.st[0], lang_only_ask(L.win[0].as<float>(), 1, R, lang_ids, n_lang, o->prompt[0])));
            HIPCHK(hipStreamSynchronize(L.st[0]->lanes[0].st));
            HIPCHK(hipMemcpy(lang_out + b0, L.st[0]->lg.out.p, (size_t)nb * 4, hipMemcpyDeviceToHost));
        }
        inits.resize((size_t)B * o->n_prompt);
        for (int b = 0; b < B; ++b) {
            std::copy(o->prompt, o->prompt + o->n_prompt, inits.begin() + (size_t)b * o->n_prompt);
            inits[(size_t)b * o->n_prompt + 1] = lang_out[b];
        }
    }
    int cursor = 0;
    for (;;) {
        for (int k = 0; k < 2; ++k) {  // fill idle states with ready utterances
            if (n_items[k]) continue;
            std::vector<int32_t>& h = L.h_items[k];
            h.clear();
            for (int i = 0; i < B && (int)h.size() < 3 * R; ++i) {
                const int b = (cursor + i) % B;
                if (busy[b] || seek[b] >= nf[b]) continue;
                snf[b] = (int)std::min<int64_t>(nf[b] - seek[b], W);
                h.insert(h.end(), {b, (int32_t)seek[b], snf[b]});
                busy[b] = 1;
            }
            if (h.empty()) continue;
            n_items[k] = (int)h.size() / 3;
            cursor = (h[3 * (n_items[k] - 1)] + 1) % B;
            for (int r = n_items[k]; r < R; ++r) h.insert(h.end(), {h[0], h[1], h[2]});
            int rc = hipMemcpyAsync(L.items[k].p, h.data(), (size_t)R * 3 * 4, hipMemcpyHostToDevice, m->stream) == hipSuccess ? 0
                     : fail(WM_E_HIP, "items upload failed");
            if (!rc) {
                launch_window_gather(mel, L.items[k].as<int>(), L.win[k].as<float>(), R, c.n_mels, T, W, m->stream);
                rc = hipGetLastError() == hipSuccess ? 0 : fail(WM_E_HIP, "window gather launch failed");
            }
            bool per_row = false;
            if (!plain) {
                row_prompts[k].assign((size_t)R * c.n_text_ctx, 0);
                row_len[k].assign(R, 0);
                for (int r = 0; r < R; ++r) {  // (spare rows repeat row 0 with its prompt)
                    const int b = h[3 * r];
                    const int32_t* init = lang_ids ? inits.data() + (size_t)b * o->n_prompt : o->prompt;  // the row's own initial ids
                    long_prompt(res->tokens[b].data(), res->segs[b].data(), (int)res->segs[b].size(), init, o->n_prompt, lo, o->timestamp_begin,
                                c.n_text_ctx, pr);
                    std::copy(pr.begin(), pr.end(), row_prompts[k].begin() + (size_t)r * c.n_text_ctx);
                    row_len[k][r] = (int32_t)pr.size();
                    per_row = per_row || lang_ids || (int)pr.size() != o->n_prompt || !std::equal(pr.begin(), pr.end(), init);
                }
            }
            row_len[k].resize(R, o->n_prompt);
            if (!per_row) {
                res->longest_prompt = std::max(res->longest_prompt, o->n_prompt);
                std::fill(row_len[k].begin(), row_len[k].end(), o->n_prompt);
                pass_total[k] = o->n_prompt + 1 + o->max_loop;
                if (!rc) rc = submit_on(m, &L.st[k], window_ask(k, o));
            } else if (!rc) {
                wm_decode_opts o2;
                RowPrompts rows;
                rc = rows_check(m, o, R, row_prompts[k].data(), row_len[k].data(), c.n_text_ctx, o2, rows);
                pass_total[k] = o2.n_prompt + 1 + o2.max_loop;
                if (!rc) {
                    res->longest_prompt = std::max(res->longest_prompt, o2.n_prompt);
                    ++res->row_passes;
                }
                if (!rc) {
                    PassAsk ask = window_ask(k, &o2);
                    ask.rows = &rows;
                    rc = submit_on(m, &L.st[k], ask);
                }
            }
            if (rc) {
                n_items[k] = 0;
                drain();
                return rc;
            }
            order[k] = ++ticket;
            ++res->passes;
            res->rows += R;
        }
        int k = -1;  // the older pass in flight
        for (int j = 0; j < 2; ++j)
            if (n_items[j] && (k < 0 || order[j] < order[k])) k = j;
        if (k < 0) break;
        const int rc = collect(k);
        const int n = n_items[k];
        n_items[k] = 0;
        if (rc) {
            drain();
            return rc;
        }
        for (int r = 0; r < n; ++r) {
            const int b = L.h_items[k][3 * r];
            const int32_t* row = toks.data() + (size_t)r * pass_total[k];
            const int n_prompt = row_len[k][r];
            int g1 = cnt[r];
            if (g1 > n_prompt && row[g1 - 1] == o->eot) --g1;  // HF drops the trailing eos
            const int g0 = std::min(n_prompt, g1);
            if (quality) {
                const bool skip = lo->use_no_speech_threshold && avg[r] < lo->logprob_threshold && nsp[r] > lo->no_speech_threshold;
                res->wins[b].push_back(wm_long_result::Window{seek[b], avg[r], nsp[r], skip ? 1 : 0});
                if (skip) {  // HF: no segments, no ids, seek += seek_num_frames (not _retrieve_segment's advance)
                    seek[b] += snf[b];
                    busy[b] = 0;
                    ++res->windows;
                    ++res->skipped;
                    continue;
                }
            }
            int adv = long_segments(row + g0, g1 - g0, o->timestamp_begin, seek[b], snf[b], segs);
            if (adv == 0) {  // the deviation: HF would decode this window again, forever
                adv = snf[b];
                ++res->stalled;
            }
            std::vector<int32_t>& seq = res->tokens[b];
            for (wm_segment sg : segs) {
                const int32_t first = (int32_t)seq.size();
                seq.insert(seq.end(), row + g0 + sg.first, row + g0 + sg.first + sg.count);
                sg.first = first;
                res->segs[b].push_back(sg);
                if (quality) {
                    res->seg_avg[b].push_back(avg[r]);
                    res->seg_nsp[b].push_back(nsp[r]);
                }
            }
            if (tt) long_slice_times(wt.data() + (size_t)r * L1, segs, res->times[b]);
            seek[b] += adv;
            busy[b] = 0;
            ++res->windows;
        }
    }
    return 0;
}

static int transcribe_long_impl(wm_model* m, const float* mel_dev, int T, const int32_t* nf, int B, const wm_decode_opts* o, wm_long_result** out,
                                const wm_long_opts* lo, const int32_t* lang_ids = nullptr, int n_lang = 0, int32_t* lang_out = nullptr,
                                bool tt = false) {
    wm_long_result* r = new wm_long_result();
    r->times.resize(B);
    r->tokens.resize(B);
    r->segs.resize(B);
    r->wins.resize(B);
    r->seg_avg.resize(B);
    r->seg_nsp.resize(B);
    const int rc = long_run(m, mel_dev, T, nf, B, o, r, lo, lang_ids, n_lang, lang_out, tt);
    (void)hipStreamSynchronize(m->stream);
    long_release(m);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return 0;
}

// the extra refusals of a long-form run with language detection; everything is refused before anything is launched
static int long_lang_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* lang_ids, int n_lang, const int32_t* lang_out) {
    if (!lang_out) return fail(WM_E_ARG, "bad argument");
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (o->n_prompt < 2) return fail(WM_E_ARG, "language detection needs at least two initial ids (<|startoftranscript|> and the language slot)");
    if (dec_lanes_for(std::min((B + 1) / 2, m->cfg.max_batch)) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    if (m->cfg.dims.n_text_ctx < o->n_prompt + 1 + o->max_loop) return fail(WM_E_ARG, "the decoder context is too short");
    return 0;
}
// the extra refusals of a long-form run with token timestamps, before anything is launched
static int long_tt_check(wm_model* m, const wm_long_opts* lo) {
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold))
        return fail(WM_E_ARG, "token timestamps do not combine with logprob_threshold / no_speech_threshold");
    if (m->align_pairs.empty()) return fail(WM_E_STATE, "token timestamps need alignment heads (wm_set_alignment_heads)");
    return 0;
}
static int long_mel_impl(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* o,
                         const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, bool want_lang, wm_long_result** out,
                         bool tt = false) {
    if (!m || !mel || !out || T <= 0) return fail(WM_E_ARG, "bad argument");
    *out = nullptr;
    WMCHK(long_check(m, o, B));
    if (tt) WMCHK(long_tt_check(m, lo));
    WMCHK(long_opts_check(lo, o->prompt, o->n_prompt, o->max_loop, m->cfg.dims.vocab, m->cfg.dims.n_text_ctx, std::min((B + 1) / 2, m->cfg.max_batch)));
    if (want_lang) WMCHK(long_lang_check(m, o, B, lang_ids, n_lang, lang_out));
    std::vector<int32_t> nf(B, T);
    if (n_frames)
        for (int b = 0; b < B; ++b) {
            if (n_frames[b] < 0 || n_frames[b] > T) return fail(WM_E_ARG, "n_frames[%d] = %d outside [0, %d]", b, n_frames[b], T);
            nf[b] = n_frames[b];
        }
    HIPCHK(hipSetDevice(m->device));
    const float* dev = mel;
    if (!mel_on_device) {
        const size_t bytes = (size_t)B * m->cfg.dims.n_mels * T * 4;
        WMCHK(grow(m->lf.in_mel, bytes));
        HIPCHK(hipMemcpyAsync(m->lf.in_mel.p, mel, bytes, hipMemcpyHostToDevice, m->stream));
        dev = m->lf.in_mel.as<float>();
    }
    return transcribe_long_impl(m, dev, T, nf.data(), B, o, out, lo, want_lang ? lang_ids : nullptr, n_lang, lang_out, tt);
}
extern "C" int wm_transcribe_long_ex(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                     const wm_decode_opts* o, const wm_long_opts* lo, wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, nullptr, 0, nullptr, false, out);
}
extern "C" int wm_transcribe_long_lang(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                       const wm_decode_opts* o, const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out,
                                       wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, lang_ids, n_lang, lang_out, true, out);
}
// lang_ids null: no language detection (lang_out is not written), else as wm_transcribe_long_lang
extern "C" int wm_transcribe_long_tt(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                     const wm_decode_opts* o, const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out,
                                     int token_timestamps, wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, lang_ids, n_lang, lang_out, lang_ids != nullptr, out, token_timestamps != 0);
}
extern "C" int wm_long_result_token_times(const wm_long_result* r, int b, double* times) {
    if (!r || b < 0 || b >= (int)r->tokens.size()) return fail(WM_E_ARG, "bad argument");
    if (!r->tt) return fail(WM_E_STATE, "this run had no token timestamps (wm_transcribe_long_tt)");
    if (!times && !r->times[b].empty()) return fail(WM_E_ARG, "bad argument");
    std::copy(r->times[b].begin(), r->times[b].end(), times);
    return 0;
}
// Host only: what a timestamp window pass and the scheduler make of one window.  rel: the window-relative fp32 time of
// each of its n generated ids (trailing eot dropped), segs: wm_op_long_segments' segments of those ids -> one float64 per kept id.
extern "C" int wm_op_long_token_times(const float* rel, int n, int64_t seek, const wm_segment* segs, int n_segs, double* times, int32_t* n_times) {
    if (n < 0 || (n > 0 && !rel) || seek < 0 || n_segs < 0 || (n_segs > 0 && !segs) || !n_times) return fail(WM_E_ARG, "bad argument");
    size_t total = 0;
    for (int i = 0; i < n_segs; ++i) {
        if (segs[i].first < 0 || segs[i].count < 0 || segs[i].first + segs[i].count > n) return fail(WM_E_ARG, "segment %d outside the window's %d ids", i, n);
        total += segs[i].count;
    }
    if (total > 0 && !times) return fail(WM_E_ARG, "bad argument");
    std::vector<double> win, kept;
    long_window_times(rel, n, seek, win);
    long_slice_times(win.data(), std::vector<wm_segment>(segs, segs + n_segs), kept);
    std::copy(kept.begin(), kept.end(), times);
    *n_times = (int32_t)kept.size();
    return 0;
}

extern "C" int wm_transcribe_long(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* o,
                                  wm_long_result** out) {
    return wm_transcribe_long_ex(m, mel, mel_on_device, B, T, n_frames, o, nullptr, out);
}

extern "C" int wm_transcribe_long_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                      wm_long_result** out) {
    return wm_transcribe_long_pcm_ex(m, pcm, n_samples, B, stride, o, nullptr, out);
}
static int long_pcm_impl(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o, const wm_long_opts* lo,
                         const int32_t* lang_ids, int n_lang, int32_t* lang_out, bool want_lang, wm_long_result** out, bool tt = false) {
    if (!m || !out) return fail(WM_E_ARG, "bad argument");
    *out = nullptr;
    WMCHK(long_check(m, o, B));
    if (tt) WMCHK(long_tt_check(m, lo));
    WMCHK(long_opts_check(lo, o->prompt, o->n_prompt, o->max_loop, m->cfg.dims.vocab, m->cfg.dims.n_text_ctx, std::min((B + 1) / 2, m->cfg.max_batch)));
    if (want_lang) WMCHK(long_lang_check(m, o, B, lang_ids, n_lang, lang_out));
    std::vector<int32_t> nf(std::max(B, 0));
    const int rc = frontend_long_run(m, pcm, n_samples, B, stride, nf.data());  // same stream as the gathers: ordered, no host sync
    if (rc) {
        (void)hipStreamSynchronize(m->stream);
        long_release(m);
        return rc;
    }
    return transcribe_long_impl(m, m->lf.mel.as<float>(), stride / FE_HOP, nf.data(), B, o, out, lo, want_lang ? lang_ids : nullptr, n_lang, lang_out, tt);
}
extern "C" int wm_transcribe_long_pcm_ex(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                         const wm_long_opts* lo, wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, nullptr, 0, nullptr, false, out);
}
extern "C" int wm_transcribe_long_pcm_lang(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                           const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, lang_ids, n_lang, lang_out, true, out);
}
extern "C" int wm_transcribe_long_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                         const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, int token_timestamps,
                                         wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, lang_ids, n_lang, lang_out, lang_ids != nullptr, out, token_timestamps != 0);
}

extern "C" int wm_long_result_sizes(const wm_long_result* r, int b, int32_t* n_tokens, int32_t* n_segments) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || !n_tokens || !n_segments) return fail(WM_E_ARG, "bad argument");
    *n_tokens = (int32_t)r->tokens[b].size();
    *n_segments = (int32_t)r->segs[b].size();
    return 0;
}
extern "C" int wm_long_result_get(const wm_long_result* r, int b, int32_t* tokens, wm_segment* segs) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || (!tokens && !r->tokens[b].empty()) || (!segs && !r->segs[b].empty()))
        return fail(WM_E_ARG, "bad argument");
    std::copy(r->tokens[b].begin(), r->tokens[b].end(), tokens);
    std::copy(r->segs[b].begin(), r->segs[b].end(), segs);
    return 0;
}
extern "C" int wm_long_result_stats(const wm_long_result* r, int32_t* windows, int32_t* stalled, int32_t* passes, int32_t* rows) {
    if (!r || !windows || !stalled || !passes || !rows) return fail(WM_E_ARG, "bad argument");
    *windows = r->windows;
    *stalled = r->stalled;
    *passes = r->passes;
    *rows = r->rows;
    return 0;
}
extern "C" int wm_long_result_prompt_stats(const wm_long_result* r, int32_t* longest_prompt, int32_t* row_passes) {
    if (!r || !longest_prompt || !row_passes) return fail(WM_E_ARG, "bad argument");
    *longest_prompt = r->longest_prompt;
    *row_passes = r->row_passes;
    return 0;
}
extern "C" int wm_long_result_quality(const wm_long_result* r, int b, float* seg_avg_logprob, float* seg_no_speech_prob) {
    if (!r || b < 0 || b >= (int)r->tokens.size()) return fail(WM_E_ARG, "bad argument");
    if (!r->quality) return fail(WM_E_STATE, "this run had no thresholds (wm_long_opts.use_logprob_threshold / use_no_speech_threshold)");
    if ((!seg_avg_logprob || !seg_no_speech_prob) && !r->segs[b].empty()) return fail(WM_E_ARG, "bad argument");
    std::copy(r->seg_avg[b].begin(), r->seg_avg[b].end(), seg_avg_logprob);
    std::copy(r->seg_nsp[b].begin(), r->seg_nsp[b].end(), seg_no_speech_prob);
    return 0;
}
extern "C" int wm_long_result_windows(const wm_long_result* r, int b, int32_t* n_windows, int64_t* seek, float* avg_logprob, float* no_speech_prob,
                                      int32_t* skipped) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || !n_windows) return fail(WM_E_ARG, "bad argument");
    if (!r->quality) return fail(WM_E_STATE, "this run had no thresholds (wm_long_opts.use_logprob_threshold / use_no_speech_threshold)");
    const std::vector<wm_long_result::Window>& w = r->wins[b];
    *n_windows = (int32_t)w.size();
    for (size_t i = 0; i < w.size(); ++i) {
        if (seek) seek[i] = w[i].seek;
        if (avg_logprob) avg_logprob[i] = w[i].avg_logprob;
        if (no_speech_prob) no_speech_prob[i] = w[i].no_speech_prob;
        if (skipped) skipped[i] = w[i].skipped;
    }
    return 0;
}
extern "C" int wm_long_result_skip_stats(const wm_long_result* r, int32_t* skipped_windows) {
    if (!r || !skipped_windows) return fail(WM_E_ARG, "bad argument");
    *skipped_windows = r->skipped;
    return 0;
}
extern "C" void wm_long_result_free(wm_long_result* r) { delete r; }
