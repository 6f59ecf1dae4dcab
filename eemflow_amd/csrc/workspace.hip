// Workspace management of the EEMFlow context (declared in ctx.h): growing device buffers and the reallocation counter that decides
// whether cached HIP graphs must go, the lazily refreshed packed weight forms, shapes, and the forward workspace.
#include <stdlib.h>

#include "ctx.h"

// bumped whenever ensure() moves a buffer: cached graphs hold workspace pointers (see alloc_workspace)
thread_local unsigned long g_realloc_events = 0;

int ensure(DevBuf& b, size_t floats) {
    if (floats > b.cap) ++g_realloc_events;
    return devbuf_ensure(b, floats);
}

// The device-resident flat weights changed (load / optimizer step): every Winograd-domain copy is stale; a launch recomputes the one it
// needs (ensure_wino) - a training step touches two forms of five layers, an inference loop one
int refresh_wino(eemflow_ctx* c, hipStream_t) {
    for (int f = 0; f < 4; ++f)
        for (int l = 0; l < ENC_NUM; ++l) c->wino_ok[f][l] = false;
    for (int l = 0; l < ENC_NUM; ++l) c->s2r_ok[l] = false;
    for (int l = 0; l < ENC_NUM; ++l) c->bx3_ok[l] = false;
    c->dec_wnc_ok = false;
    c->weights_version += 1;
    return EEM_OK;
}
int ensure_bx3(eemflow_ctx* c, int l, hipStream_t st, const float** w_out) {
    if (!c->bx3_ok[l]) {
        const int rc = bx3_transform_launch(c->flat + c->t_enc[l].w, kEncLayers[l].cin, kEncLayers[l].cout, c->wino + c->bx3_off[l], st);
        if (rc != EEM_OK) return rc;
        c->bx3_ok[l] = true;
    }
    *w_out = c->wino + c->bx3_off[l];
    return EEM_OK;
}
int ensure_s2r(eemflow_ctx* c, int l, hipStream_t st, const float** w_out) {
    if (!c->s2r_ok[l]) {
        const int rc = s2r_transform_launch(c->flat + c->t_enc[l].w, kEncLayers[l].cin, kEncLayers[l].cout, c->wino + c->s2r_off[l], st);
        if (rc != EEM_OK) return rc;
        c->s2r_ok[l] = true;
    }
    *w_out = c->wino + c->s2r_off[l];
    return EEM_OK;
}
// Winograd-domain weights of layer l (dir 0: forward, 1: data gradient) in the form the policy picks; *f4_out says which
int ensure_wino(eemflow_ctx* c, int l, int dir, int batch, hipStream_t st, const float** w_out, int* f4_out) {
    const int ch = kEncLayers[l].cin;
    const int f4 = c->layer_f4(ch, batch) ? 1 : 0;
    const int slot = f4 * 2 + dir;
    if (!c->wino_ok[slot][l]) {
        const int rc = wino_transform_launch(c->flat + c->t_enc[l].w, ch, dir, c->wino + c->wino_off[slot][l], st, f4);
        if (rc != EEM_OK) return rc;
        c->wino_ok[slot][l] = true;
    }
    *w_out = c->wino + c->wino_off[slot][l];
    *f4_out = f4;
    return EEM_OK;
}
int ensure_dec_wnc(eemflow_ctx* c, hipStream_t st) {
    if (c->dec_wnc_ok || !c->dec_wnc) return EEM_OK;
    WncPackArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < 3; ++k) {
        for (int s = 0; s < 4; ++s)
            a.job[a.njobs++] = {c->flat + c->t_dconv1[k].w, c->flat + c->t_dconv1[k].b, c->dec_wnc + c->dec_w1[k][s], c->dec_wnc + c->dec_b1[k] + 32 * s,
                                kDecW, kDecIn, 32 * s, 0};
        for (int s = 0; s < 2; ++s)
            a.job[a.njobs++] = {c->flat + c->t_dconv5[k].w, c->flat + c->t_dconv5[k].b, c->dec_wnc + c->dec_w5[k][s], c->dec_wnc + c->dec_b5[k] + 32 * s,
                                64, kDecW, 32 * s, 0};
    }
    const int rc = wnc_pack_device_launch(a, st);
    if (rc != EEM_OK) return rc;
    c->dec_wnc_ok = true;
    return EEM_OK;
}
// a training step's Winograd weights - forward and data-gradient forms of every F(4x4) layer - refreshed by ONE launch in front of its
// forward (ensure_wino then finds them valid); the F(2x2) forms stay with ensure_wino
int ensure_train_wino(eemflow_ctx* c, int batch, hipStream_t st) {
    if (!c->use_wino) return EEM_OK;
    const float* w[W4_WT_JOBS]; float* out[W4_WT_JOBS]; int ch[W4_WT_JOBS], flip[W4_WT_JOBS];
    int slot_of[W4_WT_JOBS], layer_of[W4_WT_JOBS], n = 0;
    for (int l = 0; l < ENC_NUM; ++l) {
        if (!c->enc_wino[l] || !c->layer_f4(kEncLayers[l].cin, batch)) continue;
        for (int dir = 0; dir < 2; ++dir) {
            const int slot = 2 + dir;
            if (c->wino_ok[slot][l] || n == W4_WT_JOBS) continue;
            w[n] = c->flat + c->t_enc[l].w; out[n] = c->wino + c->wino_off[slot][l]; ch[n] = kEncLayers[l].cin; flip[n] = dir;
            slot_of[n] = slot; layer_of[n] = l; ++n;
        }
    }
    if (n == 0) return EEM_OK;
    const int rc = wino4_transform_multi_launch(w, ch, flip, out, n, st);
    if (rc != EEM_OK) return rc;
    for (int i = 0; i < n; ++i) c->wino_ok[slot_of[i]][layer_of[i]] = true;
    return EEM_OK;
}

// before a graph capture / replay: the forward copies exist (a transform launched inside a capture would replay with every frame)
int ensure_forward_wino(eemflow_ctx* c, int batch, hipStream_t st) {
    { const int rcd = ensure_dec_wnc(c, st); if (rcd != EEM_OK) return rcd; }
    for (int l = 0; l < ENC_NUM; ++l) {
        const float* ws;
        if (c->enc_s2r[l] && s2r_wanted()) { const int rc = ensure_s2r(c, l, st, &ws); if (rc != EEM_OK) return rc; }
        if (c->enc_bx3[l] && bx3_wanted(l)) { const int rc = ensure_bx3(c, l, st, &ws); if (rc != EEM_OK) return rc; }
    }
    if (!c->use_wino) return EEM_OK;
    for (int l = 0; l < ENC_NUM; ++l) {
        if (!c->enc_wino[l]) continue;
        const float* w; int f4;
        const int rc = ensure_wino(c, l, 0, batch, st, &w, &f4);
        if (rc != EEM_OK) return rc;
    }
    return EEM_OK;
}

void drop_graph(eemflow_ctx* c) {
    for (eemflow_ctx::GraphEntry& e : c->graphs) {
        if (e.exec) (void)hipGraphExecDestroy(e.exec);
        if (e.graph) (void)hipGraphDestroy(e.graph);
    }
    c->graphs.clear();
}

// nimg >= 0: a stream call's encoder batch of nimg windows (Shape::nimg); -1: a forward's 2 * batch
int compute_shape(eemflow_ctx* c, int batch, int in_h, int in_w, int out_h, int out_w, Shape* s, int nimg) {
    s->batch = batch; s->in_h = in_h; s->in_w = in_w; s->out_h = out_h; s->out_w = out_w;
    s->nimg = nimg >= 0 ? nimg : 2 * batch;
    s->nimg0 = nimg >= 0 ? nimg : batch;
    s->enc_batch = nimg >= 0 ? nimg / 2 : batch;
    s->hp = in_h + c->pad[2] + c->pad[3];
    s->wp = in_w + c->pad[0] + c->pad[1];
    auto half = [](int v) { return (v - 1) / 2 + 1; };          // conv k3 s2 p1
    s->h1 = half(s->hp); s->w1 = half(s->wp);
    s->h2 = half(s->h1); s->w2 = half(s->w1);
    s->h3 = half(s->h2); s->w3 = half(s->w2);
    s->gh = s->h1 / 32; s->gw = s->w1 / 32;
    EEM_REQUIRE(s->gh >= 1 && s->gw >= 1, "input %dx%d (padded %dx%d) is too small for the 1/64 grid", in_h, in_w,
                s->hp, s->wp);
    // the reference concatenates the three decoders' flows (EEMFlow.py:179): the three pooled grids
    // must agree or torch.cat raises
    EEM_REQUIRE(s->h2 / 16 == s->gh && s->h3 / 8 == s->gh && s->w2 / 16 == s->gw && s->w3 / 8 == s->gw,
                "pooled grids of the three stages differ for padded size %dx%d (the reference's torch.cat "
                "fails too)", s->hp, s->wp);
    // stage pooling can ride in the epilogue of pconv1_2 / pconv2_3 / pconv3_3 when those run the fast path
    const int last[3] = {ENC_1_2, ENC_2_3, ENC_3_3};
    const int hs[3] = {s->h1, s->h2, s->h3}, ws[3] = {s->w1, s->w2, s->w3}, ks[3] = {32, 16, 8};
    for (int k = 0; k < 3; ++k) {
        const EncLayerDesc& d = kEncLayers[last[k]];
        int th, tw, pk;
        const bool wino = c->use_wino && c->enc_wino[last[k]] && wino_supported(d.cin, d.cout, d.stride, ws[k]);
        if (wino) wino_tile(d.cin, c->layer_f4(d.cin, s->enc_batch) ? 1 : 0, &th, &tw, &pk);
        else enc2_tile(d.cin, d.cout, &th, &tw, &pk);
        s->fuse[k] = (wino || (c->enc_has2[last[k]] && enc2_supported(d.cin, d.cout, d.stride, ws[k]))) && pk == ks[k];
        s->th[k] = th;
        s->prow[k] = ceil_div(hs[k], th);
        s->pcol[k] = ceil_div(ws[k], tw) * (tw / ks[k]);
    }
    return EEM_OK;
}

int alloc_workspace_raw(eemflow_ctx* c, const Shape& s);
// workspace for shape s; cached graphs survive unless a buffer had to move
int alloc_workspace(eemflow_ctx* c, const Shape& s) {
    const unsigned long before = g_realloc_events;
    const int rc = alloc_workspace_raw(c, s);
    if (g_realloc_events != before) drop_graph(c);
    return rc;
}

int alloc_workspace_raw(eemflow_ctx* c, const Shape& s) {
    const size_t n2 = (size_t)s.nimg, B = s.batch, g = (size_t)s.gh * s.gw;
    int rc;
#define ENS(buf, n) if ((rc = ensure(buf, n)) != EEM_OK) return rc
    ENS(c->a1, n2 * 16 * s.h1 * s.w1);  ENS(c->f11, n2 * 16 * s.h1 * s.w1);
    ENS(c->a2, n2 * 32 * s.h2 * s.w2);  ENS(c->b2, n2 * 32 * s.h2 * s.w2);  ENS(c->f12, n2 * 32 * s.h2 * s.w2);
    ENS(c->a3, n2 * 64 * s.h3 * s.w3);  ENS(c->b3, n2 * 64 * s.h3 * s.w3);  ENS(c->f13, n2 * 64 * s.h3 * s.w3);
    const int pc[3] = {16, 32, 64};
    for (int k = 0; k < 3; ++k) {
        ENS(c->pool[k], n2 * pc[k] * g);
        if (s.fuse[k]) ENS(c->ppart[k], n2 * pc[k] * (size_t)s.prow[k] * s.pcol[k]);
        ENS(c->cat[k], B * kDecIn * g);
        ENS(c->ta[k], B * kDecW * g);   ENS(c->tb[k], B * kDecW * g);
        ENS(c->tc[k], B * kDecW * g);   ENS(c->td[k], B * kDecW * g);
        ENS(c->t64[k], B * 64 * g);     ENS(c->t32[k], B * 32 * g);
    }
    ENS(c->flowcat, B * 6 * g);  ENS(c->coarse, B * 2 * g);
    if (c->enc0_generic) { ENS(c->padded, n2 * c->cin0 * (size_t)s.hp * s.wp); }
    else {                                                   // block scratch of the OPT-IN fused first two layers only (41 MB)
        if (sw_on<SW_EEM_FUSE12>()) { ENS(c->fuse_scratch, enc12_scratch_floats(256)); }
    }
#undef ENS
    return EEM_OK;
}
