// wm_score.cpp — transcript scoring and forced alignment: the teacher-forced pass, its collection, the
// wm_score*, wm_score_nbest*  and wm_align* entries, and wm_op_score_logits / wm_op_score_rank.
#include "wm_runtime.h"

// ---- transcript scoring --------------------------------------------------------------------------------------------
// Row b holds ids y[0 .. len_b); its decoder input is y[0 .. len_b - 1), run through the per-row prefill's position-major chunks
// (left-padded so that the rows end together, key windows as in §16) with no logits launch; after every chunk the real rows of the
// last layer's residual stream are copied out, utterance-major; then one LayerNorm launch, one vocabulary sweep and the merge.
// Everything is refused before anything is launched.
static int score_check(wm_model* m, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len) {
    if (!m || !ids || !ids_len || B <= 0 || ids_stride < 2) return fail(WM_E_ARG, "bad argument");
    if (pos_mode != WM_POS_REF && pos_mode != WM_POS_HF) return fail(WM_E_ARG, "bad pos_mode");
    const wm_dims& c = m->cfg.dims;
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "scoring needs a single-lane decode state");
    const int cap = std::min(ids_stride, c.n_text_ctx);
    for (int b = 0; b < B; ++b) {
        const int L = ids_len[b], cl = context_len ? context_len[b] : 1;
        if (L < 2 || L > cap) return fail(WM_E_ARG, "ids_len[%d] = %d outside [2, min(ids_stride, n_text_ctx) = %d]", b, L, cap);
        if (cl < 1 || cl > L - 1) return fail(WM_E_ARG, "context_len[%d] = %d outside [1, ids_len - 1 = %d]", b, cl, L - 1);
        for (int i = 0; i < L; ++i) {
            const int32_t id = ids[(size_t)b * ids_stride + i];
            if (id < 0 || id >= c.vocab) return fail(WM_E_ARG, "id %d of row %d out of range", id, b);
        }
    }
    return 0;
}
int score_pass(wm_model* m, wm_state* s, const ScoreAsk& a) {
    const wm_dims& c = m->cfg.dims;
    const int B = s->B, T = dec_dtype(m->cfg);
    const size_t d = c.d_model;
    wm_state::Score& sc = s->sc;
    int Lmax = 0, M = 0;
    for (int b = 0; b < B; ++b) {
        Lmax = std::max(Lmax, a.len[b] - 1);
        M += a.len[b] - 1;
    }
    sc.M = M;
    sc.Lmax = Lmax;
    sc.stride = a.stride;
    sc.h_tok.assign((size_t)Lmax * B, 0);
    sc.h_pos.assign((size_t)Lmax * B, 0);
    sc.h_dst.assign((size_t)Lmax * B, -1);
    sc.h_key_lo.assign(B, 0);
    sc.h_target.assign(M, -1);
    sc.h_slot.assign(M, 0);
    sc.h_len.assign(a.len, a.len + B);
    sc.h_ctx.assign(B, 1);
    // an align pass: the cross-q rows of inputs t in [context_len, len - 1) are captured, R_b = len_b - context_len_b - 1
    const bool align = a.cols != nullptr, want_lp = !align || a.lp;
    wm_state::Align& al = s->al;
    int Lal = 0;
    if (align) {
        al.h_rows.assign(B, 0);
        al.h_row0.assign(B, 1);
        for (int b = 0; b < B; ++b) {
            al.h_row0[b] = a.ctx ? a.ctx[b] : 1;
            al.h_rows[b] = a.len[b] - al.h_row0[b] - 1;
            Lal = std::max(Lal, al.h_rows[b]);
        }
        al.h_map.assign((size_t)Lmax * B, -1);
    }
    for (int b = 0, base = 0; b < B; ++b) {
        const int n_in = a.len[b] - 1, pad = Lmax - n_in, cl = a.ctx ? a.ctx[b] : 1;
        const int32_t* y = a.ids + (size_t)b * a.stride;
        sc.h_ctx[b] = cl;
        sc.h_key_lo[b] = pad;
        for (int t = 0; t < Lmax; ++t) {
            const size_t o = (size_t)t * B + b;
            if (t < pad) {  // a dead slot in front of a shorter row: the row's first id at position 0, never attended to (§16)
                sc.h_tok[o] = y[0];
                continue;
            }
            const int i = t - pad;
            sc.h_tok[o] = y[i];
            // WM_POS_REF: the reference's loop feeds position current_len - 1 (whisper.mojo:217), as set_rows_step_kernel applies it
            sc.h_pos[o] = a.pos_mode == WM_POS_REF && i >= cl ? i - 1 : i;
            sc.h_dst[o] = base + i;
            if (align && i >= cl) al.h_map[o] = b * Lal + (i - cl);
            sc.h_target[base + i] = y[i + 1];
            sc.h_slot[base + i] = b * a.stride + i + 1;
        }
        base += n_in;
    }
    int spp = 0;
    const size_t parts = score_parts(c.vocab, T, &spp), ctx = c.n_text_ctx;
    WMCHK(grow(s->rw.key_lo, (size_t)B * 4));
    WMCHK(grow(s->tok_rows, (size_t)B * ctx * 4));
    WMCHK(grow(s->pos_rows, (size_t)B * ctx * 4));
    if (want_lp) {
        WMCHK(grow(sc.rows, (size_t)M * d * 4));
        WMCHK(grow(sc.a, score_operand_bytes(M, c.d_model, T)));
        for (DevBuf* p : {&sc.pmax, &sc.psum, &sc.pidx}) WMCHK(grow(*p, (size_t)M * parts * 4));
        for (DevBuf* p : {&sc.ztgt, &sc.target, &sc.slot}) WMCHK(grow(*p, (size_t)M * 4));
        WMCHK(grow(sc.dst, (size_t)B * ctx * 4));
        for (DevBuf* p : {&sc.len, &sc.ctx, &sc.sum, &sc.avg}) WMCHK(grow(*p, (size_t)B * 4));
        for (DevBuf* p : {&sc.lp, &sc.top}) WMCHK(grow(*p, (size_t)B * a.stride * 4));
    }
    // an n-best pass: row r's cross-attention reads clip utt_of[r]; the ranking runs per clip over rows row0 .. + n_cand
    wm_state::Nbest& nb = s->nb;
    const bool nbest = a.n_utt > 0;
    if (nbest) {
        nb.U = a.n_utt;
        nb.h_n_cand.assign(a.n_cand, a.n_cand + a.n_utt);
        nb.h_row0.assign(a.n_utt, 0);
        nb.h_utt_of.assign(B, 0);
        for (int u = 0, r = 0; u < a.n_utt; ++u) {
            nb.h_row0[u] = r;
            for (int k = 0; k < a.n_cand[u]; ++k) nb.h_utt_of[r++] = u;
        }
        for (DevBuf* p : {&nb.utt_of, &nb.order, &nb.post}) WMCHK(grow(*p, (size_t)B * 4));
        for (DevBuf* p : {&nb.row0, &nb.n_cand, &nb.best}) WMCHK(grow(*p, (size_t)a.n_utt * 4));
    }
    al.on = al.ragged = align;
    al.win = false;
    if (align) {  // the buffers of a timestamp pass, sized by the longest row of THIS pass
        al.pairs = m->align_pairs;
        al.L = Lal;
        al.n_prompt = 0;
        al.stride = a.stride;
        al.cols = *a.cols;
        ++al.gen;
        invalidate_step_graphs(s);  // the captured step graph may hold a capture into a buffer that is re-sized here
        WMCHK(align_buffers(m, s, std::max(Lal, 1), a.stride));
        for (DevBuf* p : {&al.rows, &al.row0}) WMCHK(grow(*p, (size_t)B * 4));
        WMCHK(grow(al.map, (size_t)B * ctx * 4));
    }
    s->rw.on = true;  // the prefill's self-attention sweeps each row's own key window
    s->rw.Lmax = Lmax;
    sc.on = true;
    nb.on = nbest;
    const wm_state::Lane& ln = s->lanes[0];
    const DecView v{ln.b0, ln.nb, ln.st, ln.ctl};
    HIPCHK(hipEventRecord(s->enc_done, s->enc_stream ? s->enc_stream : m->stream));
    HIPCHK(hipStreamWaitEvent(v.st, s->enc_done, 0));
    auto up = [&](DevBuf& dst, const std::vector<int32_t>& h) { return hipMemcpyAsync(dst.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, v.st); };
    HIPCHK(up(s->tok_rows, sc.h_tok));
    HIPCHK(up(s->pos_rows, sc.h_pos));
    HIPCHK(up(s->rw.key_lo, sc.h_key_lo));
    if (want_lp) {
        HIPCHK(up(sc.dst, sc.h_dst));
        HIPCHK(up(sc.target, sc.h_target));
        HIPCHK(up(sc.slot, sc.h_slot));
        HIPCHK(up(sc.len, sc.h_len));
        HIPCHK(up(sc.ctx, sc.h_ctx));
        HIPCHK(hipMemsetAsync(sc.lp.p, 0, (size_t)B * a.stride * 4, v.st));     // logprob[b][0] and the tails: 0
        HIPCHK(hipMemsetAsync(sc.top.p, 0xff, (size_t)B * a.stride * 4, v.st));  // top_id[b][0] and the tails: -1
    }
    if (nbest) {
        HIPCHK(up(nb.utt_of, nb.h_utt_of));
        HIPCHK(up(nb.row0, nb.h_row0));
        HIPCHK(up(nb.n_cand, nb.h_n_cand));
    }
    if (align) {  // (the host vectors outlive the copies: the state is not reused before this pass is waited for)
        HIPCHK(up(al.map, al.h_map));
        HIPCHK(up(al.rows, al.h_rows));
        HIPCHK(up(al.row0, al.h_row0));
        HIPCHK(up(al.ncols, al.cols));
    }
    HIPCHK(hipEventRecord(sc.ev[1], v.st));
    trace_mark(v.st, "state %p score prefill start", (void*)s);
    for (int t0 = 0; t0 < Lmax; t0 += wm_state::PREFILL_MAX) {
        const int P = std::min<int>(wm_state::PREFILL_MAX, Lmax - t0);
        launch_set_step(v.ctl, t0, 1, nullptr, 0, nullptr, 0, v.nb, v.st);
        DecPass chunk;
        chunk.P = P;
        chunk.t0 = t0;
        chunk.capture = align && Lal > 0;
        WMCHK(decode_core(m, s, v, chunk));
        if (want_lp) launch_score_collect(s->dx.as<float>(), sc.rows.as<float>(), sc.dst.as<int>() + (size_t)t0 * B, P * B, c.d_model, v.st);
    }
    HIPCHK(hipEventRecord(sc.ev[2], v.st));
    trace_mark(v.st, "state %p score prefill end", (void*)s);
    if (!want_lp) {  // times only: no LayerNorm, sweep, merge or sums
        for (int k = 3; k <= 5; ++k) HIPCHK(hipEventRecord(sc.ev[k], v.st));
    } else {
    const VocabHead h = vocab_head(m);
    ScoreParams q{};
    q.x = sc.rows.as<float>();
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.a = sc.a.p;
    q.target = sc.target.as<int>();
    q.slot = sc.slot.as<int>();
    q.M = M;
    q.N = h.vocab;
    q.K = h.d_model;
    q.pmax = sc.pmax.as<float>();
    q.psum = sc.psum.as<float>();
    q.pidx = sc.pidx.as<int>();
    q.ztgt = sc.ztgt.as<float>();
    q.logprob = sc.lp.as<float>();
    q.top_id = sc.top.as<int>();
    int lrc = 0;
    DISPATCH_DT(T, TT, lrc = launch_score<TT>(q, v.st, sc.ev + 3));
    LCHK(lrc);
    launch_score_sums(sc.lp.as<float>(), a.stride, sc.len.as<int>(), sc.ctx.as<int>(), sc.sum.as<float>(), sc.avg.as<float>(), B, v.st);
    if (nbest)  // ranking and posterior per clip, behind the sums on the same stream
        launch_score_rank(ScoreRankParams{a.normalize ? sc.avg.as<float>() : sc.sum.as<float>(), nb.row0.as<int>(), nb.n_cand.as<int>(),
                                          nb.order.as<int>(), nb.best.as<int>(), nb.post.as<float>()}, nb.U, v.st);
    HIPCHK(hipEventRecord(sc.ev[5], v.st));
    }
    if (align) {  // the align chain on the lane's stream, before the pass's completion event
        WMCHK(enqueue_align(m, s));
        HIPCHK(hipEventRecord(sc.ev[6], v.st));
    }
    trace_mark(v.st, "state %p score end", (void*)s);
    HIPCHK(hipEventRecord(ln.done, ln.st));
    HIPCHK(hipGetLastError());
    s->enq_rc = 0;
    s->enq_done.store(true);
    return 0;
}
int score_collect(wm_model* m, wm_state* s, const PassOut& out) {
    if (!s || !s->pending || !s->sc.on) return fail(WM_E_STATE, "no score pass was submitted on this slot");
    HIPCHK(hipSetDevice(m->device));
    const bool align = s->al.on;  // an align pass: out.token_times [B][stride] too, the log-probs only if it computed them
    const hipError_t e = hipEventSynchronize(s->lanes[0].done);
    s->pending = false;  // afterwards the state holds no usable pass, exactly as after wm_transcribe
    s->has_enc = false;
    s->sc.on = false;
    s->rw.on = false;
    s->al.on = false;
    const bool nbest = s->nb.on;
    s->nb.on = false;
    HIPCHK(e);
    s->sc.timed = true;
    s->sc.timed_al = align;
    const size_t n = (size_t)s->B * s->sc.stride * 4;
    if (out.token_times) HIPCHK(hipMemcpy(out.token_times, s->al.times.p, n, hipMemcpyDeviceToHost));
    if (!out.token_logprobs) return 0;
    HIPCHK(hipMemcpy(out.token_logprobs, s->sc.lp.p, n, hipMemcpyDeviceToHost));
    if (out.top_ids) HIPCHK(hipMemcpy(out.top_ids, s->sc.top.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.sum_logprob, s->sc.sum.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.avg_logprob, s->sc.avg.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
    if (nbest && out.order) {  // (the n-best entries ask for the three together)
        HIPCHK(hipMemcpy(out.order, s->nb.order.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.best, s->nb.best.p, (size_t)s->nb.U * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.posterior, s->nb.post.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}
// the request and the outputs of a checked score / align call (a: the caller's ScoreAsk, alive for the call)
static PassAsk score_ask(const float* mel, int mel_on_device, int B, const ScoreAsk& a) {
    PassAsk ask{mel, mel_on_device, B};
    ask.score = &a;
    return ask;
}
static PassOut score_out(float* token_times, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    PassOut out;
    out.token_times = token_times;
    out.token_logprobs = token_logprobs;
    out.top_ids = top_ids;
    out.sum_logprob = sum_logprob;
    out.avg_logprob = avg_logprob;
    return out;
}
extern "C" int wm_score(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                        int ids_stride, const int32_t* context_len, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    if (!m || !mel || !token_logprobs || !sum_logprob || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return run_now(m, score_ask(mel, mel_on_device, B, a), score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}
extern "C" int wm_score_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids,
                               const int32_t* ids_len, int ids_stride, const int32_t* context_len) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return submit_slot(m, slot, score_ask(mel, mel_on_device, B, a));
}
extern "C" int wm_score_wait(wm_model* m, int slot, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::score, score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}
extern "C" int wm_score_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                            const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_logprobs, int32_t* top_ids,
                            float* sum_logprob, float* avg_logprob) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream order as the encoder: no host sync
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return run_now(m, score_ask(m->fe.mel.as<float>(), 1, B, a), score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}

// ---- n-best scoring -------------------------------------------------------------------------------------------------
// U clips, n_cand[u] candidate rows each (R rows in all, grouped by clip): the encoder and the cross-K/V projection run over the U
// clips, the decoder over the R rows, each row's cross-attention reading its clip's X or K/V by row map; per row exactly what wm_score
// gives with the clip's mel repeated, per clip a ranking and a posterior made on the device.  Everything is refused before anything is
// launched; *R_out = Σ n_cand.
static int nbest_check(wm_model* m, int U, const int32_t* n_cand, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride,
                       const int32_t* context_len, int* R_out) {
    if (!m || !n_cand || U < 1) return fail(WM_E_ARG, "bad argument (U >= 1 clips, n_cand[U])");
    long R = 0;
    for (int u = 0; u < U; ++u) {
        if (n_cand[u] < 1) return fail(WM_E_ARG, "n_cand[%d] = %d: every clip needs at least one candidate", u, n_cand[u]);
        R += n_cand[u];
        if (R > m->cfg.max_batch) return fail(WM_E_ARG, "%d clips hold more than max_batch %d candidates", U, m->cfg.max_batch);
    }
    WMCHK(score_check(m, (int)R, pos_mode, ids, ids_len, ids_stride, context_len));
    *R_out = (int)R;
    return 0;
}
static ScoreAsk nbest_ask(int U, const int32_t* n_cand, int normalize, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride,
                          const int32_t* context_len) {
    ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    a.n_utt = U;
    a.n_cand = n_cand;
    a.normalize = normalize != 0;
    return a;
}
static PassOut nbest_out(float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob, int32_t* order, int32_t* best,
                         float* posterior) {
    PassOut out = score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob);
    out.order = order;
    out.best = best;
    out.posterior = posterior;
    return out;
}
extern "C" int wm_score_nbest(wm_model* m, const float* mel, int mel_on_device, int U, const int32_t* n_cand, int normalize, int pos_mode,
                              const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_logprobs,
                              int32_t* top_ids, float* sum_logprob, float* avg_logprob, int32_t* order, int32_t* best, float* posterior) {
    if (!m || !mel || !token_logprobs || !sum_logprob || !avg_logprob || !order || !best || !posterior) return fail(WM_E_ARG, "bad argument");
    int R = 0;
    WMCHK(nbest_check(m, U, n_cand, pos_mode, ids, ids_len, ids_stride, context_len, &R));
    const ScoreAsk a = nbest_ask(U, n_cand, normalize, pos_mode, ids, ids_len, ids_stride, context_len);
    return run_now(m, score_ask(mel, mel_on_device, R, a), nbest_out(token_logprobs, top_ids, sum_logprob, avg_logprob, order, best, posterior));
}
extern "C" int wm_score_nbest_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int U, const int32_t* n_cand, int normalize,
                                     int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    int R = 0;
    WMCHK(nbest_check(m, U, n_cand, pos_mode, ids, ids_len, ids_stride, context_len, &R));
    const ScoreAsk a = nbest_ask(U, n_cand, normalize, pos_mode, ids, ids_len, ids_stride, context_len);
    return submit_slot(m, slot, score_ask(mel, mel_on_device, R, a));
}
extern "C" int wm_score_nbest_wait(wm_model* m, int slot, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob,
                                   int32_t* order, int32_t* best, float* posterior) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob || !order || !best || !posterior || slot < 0 || slot >= wm_model::NSLOT)
        return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::nbest, nbest_out(token_logprobs, top_ids, sum_logprob, avg_logprob, order, best, posterior));
}
extern "C" int wm_score_nbest_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int U, int stride, const int32_t* n_cand,
                                  int normalize, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride,
                                  const int32_t* context_len, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob,
                                  int32_t* order, int32_t* best, float* posterior) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob || !order || !best || !posterior) return fail(WM_E_ARG, "bad argument");
    int R = 0;
    WMCHK(nbest_check(m, U, n_cand, pos_mode, ids, ids_len, ids_stride, context_len, &R));
    WMCHK(frontend_run(m, pcm, n_samples, U, stride));  // same stream order as the encoder: no host sync
    const ScoreAsk a = nbest_ask(U, n_cand, normalize, pos_mode, ids, ids_len, ids_stride, context_len);
    return run_now(m, score_ask(m->fe.mel.as<float>(), 1, R, a),
                   nbest_out(token_logprobs, top_ids, sum_logprob, avg_logprob, order, best, posterior));
}
// The ranking launch alone on host keys: known-answer tests.
extern "C" int wm_op_score_rank(int32_t* order, int32_t* best, float* posterior, const float* key, const int32_t* n_cand, int U) {
    if (!order || !best || !posterior || !key || !n_cand || U < 1) return fail(WM_E_ARG, "bad argument");
    std::vector<int32_t> row0(U);
    long R = 0;
    for (int u = 0; u < U; ++u) {
        if (n_cand[u] < 1) return fail(WM_E_ARG, "n_cand[%d] = %d: every clip needs at least one candidate", u, n_cand[u]);
        row0[u] = (int32_t)R;
        R += n_cand[u];
        if (R > (1 << 20)) return fail(WM_E_ARG, "more than 2^20 candidates");
    }
    for (long r = 0; r < R; ++r)
        if (!std::isfinite(key[r])) return fail(WM_E_ARG, "key[%ld] is not finite (the counting rank needs comparable keys)", r);
    TmpDev t;
    DevBuf &dk = t.add(), &d0 = t.add(), &dn = t.add(), &dor = t.add(), &db = t.add(), &dp = t.add();
    WMCHK(upload_bytes(dk, key, (size_t)R * 4));
    WMCHK(upload_bytes(d0, row0.data(), (size_t)U * 4));
    WMCHK(upload_bytes(dn, n_cand, (size_t)U * 4));
    for (DevBuf* p : {&dor, &dp}) WMCHK(p->alloc((size_t)R * 4, true));
    WMCHK(db.alloc((size_t)U * 4, true));
    launch_score_rank(ScoreRankParams{dk.as<float>(), d0.as<int>(), dn.as<int>(), dor.as<int>(), db.as<int>(), dp.as<float>()}, U, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(order, dor.p, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(best, db.p, (size_t)U * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(posterior, dp.p, (size_t)R * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int wm_score_phases(wm_model* m, int slot, float* ms) {
    if (!m || !ms || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    wm_state* s = *slot_state(m, slot);
    if (!s || !state_is_live(s) || s->pending || !s->sc.timed) return fail(WM_E_STATE, "no completed score pass on this slot's state");
    HIPCHK(hipSetDevice(m->device));
    for (int k = 0; k < 5; ++k) HIPCHK(hipEventElapsedTime(ms + k, s->sc.ev[k], s->sc.ev[k + 1]));
    return 0;
}

// ---- forced alignment ------------------------------------------------------------------------------------------------
// Token timestamps of a GIVEN transcript: the score pass with the alignment layers' cross-q rows captured by row map, then the align
// chain with per-row row counts and offsets.  token_logprobs / sum_logprob / avg_logprob are nullable as a group: without them the
// vocabulary side is not launched.  Everything is refused before anything is launched.
static int align_check(wm_model* m, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len,
                       const int32_t* n_frames, const float* token_logprobs, const float* sum_logprob, const float* avg_logprob,
                       std::vector<int32_t>& cols) {
    if ((token_logprobs != nullptr) != (sum_logprob != nullptr) || (token_logprobs != nullptr) != (avg_logprob != nullptr))
        return fail(WM_E_ARG, "token_logprobs, sum_logprob and avg_logprob go together");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    return align_cols(m, n_frames, B, cols);
}
extern "C" int wm_align(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                        int ids_stride, const int32_t* context_len, const int32_t* n_frames, float* token_times, float* token_logprobs,
                        float* sum_logprob, float* avg_logprob) {
    if (!m || !mel || !token_times) return fail(WM_E_ARG, "bad argument");
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, n_frames, token_logprobs, sum_logprob, avg_logprob, cols));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, token_logprobs != nullptr};
    return run_now(m, score_ask(mel, mel_on_device, B, a), score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
extern "C" int wm_align_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids,
                               const int32_t* ids_len, int ids_stride, const int32_t* context_len, const int32_t* n_frames, int want_logprobs) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, n_frames, nullptr, nullptr, nullptr, cols));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, want_logprobs != 0};
    return submit_slot(m, slot, score_ask(mel, mel_on_device, B, a));
}
extern "C" int wm_align_wait(wm_model* m, int slot, float* token_times, float* token_logprobs, float* sum_logprob, float* avg_logprob) {
    if (!m || !token_times || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    if ((token_logprobs != nullptr) != (sum_logprob != nullptr) || (token_logprobs != nullptr) != (avg_logprob != nullptr))
        return fail(WM_E_ARG, "token_logprobs, sum_logprob and avg_logprob go together");
    return collect_slot(m, slot, PassKind::align, score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
// n_frames from the sample counts, as wm_transcribe_pcm_tt
extern "C" int wm_align_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                            const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_times, float* token_logprobs,
                            float* sum_logprob, float* avg_logprob) {
    if (!m || !token_times || !n_samples || B <= 0) return fail(WM_E_ARG, "bad argument");
    std::vector<int32_t> nf(B);
    for (int b = 0; b < B; ++b) nf[b] = (int32_t)std::min<long>(2L * m->cfg.dims.n_audio_ctx, ((long)n_samples[b] + FE_HOP - 1) / FE_HOP);
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, nf.data(), token_logprobs, sum_logprob, avg_logprob, cols));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream order as the encoder: no host sync
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, token_logprobs != nullptr};
    return run_now(m, score_ask(m->fe.mel.as<float>(), 1, B, a), score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
// ms[6]: wm_score_phases' five (LayerNorm, sweep and merge are 0 for a pass without log-probs) and the align chain
extern "C" int wm_align_phases(wm_model* m, int slot, float* ms) {
    if (!m || !ms || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    wm_state* s = *slot_state(m, slot);
    if (!s || !state_is_live(s) || s->pending || !s->sc.timed_al) return fail(WM_E_STATE, "no completed align pass on this slot's state");
    HIPCHK(hipSetDevice(m->device));
    for (int k = 0; k < 6; ++k) HIPCHK(hipEventElapsedTime(ms + k, s->sc.ev[k], s->sc.ev[k + 1]));
    return 0;
}
// The score pass's vocabulary side alone (LayerNorm, sweep, merge) on host operands: known-answer tests.
extern "C" int wm_op_score_logits(float* logprob, int32_t* top_id, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                                  const int32_t* target, int M, int N, int K, int dtype) {
    if (!logprob || !top_id || !x || !ln_g || !ln_b || !emb || !target || M <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(vocab_k_check(K));
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    for (int r = 0; r < M; ++r)
        if (target[r] >= N) return fail(WM_E_ARG, "target[%d] = %d is not a vocabulary id", r, target[r]);
    TmpDev t;
    const size_t parts = score_parts(N, dtype);
    const float* dx;
    VocabHead vh;
    WMCHK(upload_vocab_head(t, x, ln_g, ln_b, emb, M, N, K, dtype, &dx, &vh));
    DevBuf &a = t.add(), &pm = t.add(), &ps = t.add(), &pi = t.add(), &zt = t.add(), &tg = t.add(), &lp = t.add(), &top = t.add();
    WMCHK(a.alloc(score_operand_bytes(M, K, dtype)));
    for (DevBuf* p : {&pm, &ps, &pi}) WMCHK(p->alloc((size_t)M * parts * 4, true));
    for (DevBuf* p : {&zt, &lp, &top}) WMCHK(p->alloc((size_t)M * 4, true));
    WMCHK(upload_bytes(tg, target, (size_t)M * 4));
    ScoreParams q{};
    q.x = dx;
    q.ln_g = vh.ln_g;
    q.ln_b = vh.ln_b;
    q.emb = vh.emb;
    q.a = a.p;
    q.target = tg.as<int>();
    q.M = M;
    q.N = N;
    q.K = K;
    q.pmax = pm.as<float>();
    q.psum = ps.as<float>();
    q.pidx = pi.as<int>();
    q.ztgt = zt.as<float>();
    q.logprob = lp.as<float>();
    q.top_id = top.as<int>();
    int lrc = 0;
    DISPATCH_DT(dtype, TT, lrc = launch_score<TT>(q, nullptr));
    LCHK(lrc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(logprob, lp.p, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(top_id, top.p, (size_t)M * 4, hipMemcpyDeviceToHost));
    return 0;
}
