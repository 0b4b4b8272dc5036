// Part of libbde2vid's host side, included by bde_api.hip (one translation unit: the kernels of the headers it includes are
// emitted once).  The forward's launch schedule (V5.py:100-241): convolution / recurrent / attention / decoder stages, workspaces, graph capture, serving mode, range guard.
#pragma once
namespace bde {

// ------------------------------------------------------------------------------------------
// conv launch helper
// ------------------------------------------------------------------------------------------
struct ConvCall {
    const PackedLayer* pl = nullptr;
    const float* in = nullptr;
    float* out = nullptr;
    const float* res1 = nullptr;
    const float* res2 = nullptr;
    int N = 1, Hs = 0, Ws = 0;   // input dims
    int stride = 1;
    int act = ACT_NONE;
    long in_gs = 0, out_gs = 0;  // group strides (0 = shared input)
    int mask_w = 0, mask_pt = 0, mask_pl = 0;
    int cout_rows = -1;          // override (kvall uses all rows)
    const float* pred_head = nullptr;   // fused predI (conv_mfma.h): set pred_out to enable
    float* pred_out = nullptr;
    float* out_sb = nullptr;     // store the result as SB16 here INSTEAD of fp32 planes in `out` (conv_mfma.h sb_out)
    long out_sb_gs = 0;          // its group stride, floats
    bool in_sb = false;          // `in` already is the SB16 image (in_gs in floats of that image): conv_sb or fail
    int decide_N = 0;            // > 0: choose the kernel as for a launch of this many frames (a chunk of a batched launch computes
                                 // exactly what the whole launch computes for its frames)
};

// Will run_conv take the split-bf16 kernels for this layer at this size?  (decided before the producer of its input runs)
static bool conv_takes_sb(const bde_model* m, const PackedLayer& pl, int stride, int N, int Hs, int Ws) {
    const int pad = pl.KS / 2;
    const int Ho = (Hs + 2 * pad - pl.KS) / stride + 1, Wo = (Ws + 2 * pad - pl.KS) / stride + 1;
    return m->conv_sb && pl.split_off(m->sb_terms) >= 0 && conv_sb_fits(pl.KS, stride, pl.Cout, Ws, Ho, Wo, m->sb_terms) &&
           (long)(pl.G_decide ? pl.G_decide : pl.G) * N * Ho * Wo >= 16384;
}

static int run_conv(const bde_model* m, const ConvCall& cc, hipStream_t s) {
    const PackedLayer& pl = *cc.pl;
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.in = cc.in;
    a.wpk = m->P(pl.w_off);
    a.bias = m->P(pl.b_off);
    a.lnsum = pl.s_off >= 0 ? m->P(pl.s_off) : nullptr;
    a.res1 = cc.res1;
    a.res2 = cc.res2;
    a.out = cc.out;
    a.N = cc.N;
    a.Cin = pl.Cin;
    a.Hs = cc.Hs;
    a.Ws = cc.Ws;
    a.Hin = cc.Hs;
    a.Win = cc.Ws;
    a.Cout = pl.Cout;
    const int pad = pl.KS / 2;
    a.Ho = (a.Hin + 2 * pad - pl.KS) / cc.stride + 1;
    a.Wo = (a.Win + 2 * pad - pl.KS) / cc.stride + 1;
    a.nchunks = pl.nchunks;
    a.act = cc.act;
    a.mask_w = cc.mask_w;
    a.mask_pt = cc.mask_pt;
    a.mask_pl = cc.mask_pl;
    const long in_fs = (long)pl.Cin * cc.Hs * cc.Ws, out_fs = (long)pl.Cout * a.Ho * a.Wo;
    a.in_ns = in_fs;
    a.out_ns = a.res1_ns = a.res2_ns = out_fs;
    a.in_gs = cc.in_gs;
    a.out_gs = cc.out_gs;
    a.res1_gs = a.res2_gs = cc.out_gs;
    a.w_gs = pl.w_sz;
    a.bias_gs = pl.Cout;
    a.xcd_remap = m->xcd_remap;
    a.decide_groups = pl.G_decide;
    if (cc.out_sb) {
        a.sb_out = reinterpret_cast<unsigned short*>(cc.out_sb);
        a.sb_out_ns = (long)cdiv(pl.Cout, 16) * a.Ho * a.Wo * (16 * m->sb_terms);
        a.sb_out_gs = cc.out_sb_gs * 2;
        a.sb_ovf = m->ovf();
    }
    a.sb_terms = m->sb_terms;
    if (cc.pred_out) {
        a.pred_w = m->P(m->predw_off);
        a.pred_b = m->P(m->predb_off);
        a.pred_head = cc.pred_head;
        a.pred_out = cc.pred_out;
        a.pred_sigmoid = m->cfg.activation;
    }
    if (pl.KS == 1) return pw_launch_auto(a, pl.G, s);
    // (measured at the canonical sizes, us: 3x3 gate convs 530 / 497 / 505 against 954 / 954 / 989 on the fp32 matrix path;
    //  5x5: decoder 0 488 vs 633, decoder 1 (64 channels) 502 vs 641, encoder 1 / 2 (stride 2) 271 / 300 vs 345 / 335;
    //  conv_sb_pick has no shape for 32 output channels or for the stride-2 halo of level 0, those stay on the fp32 kernels)
    // (the fused predI epilogue needs every output channel of a pixel in one wave: 32 channels)
    if (cc.in_sb || ((!cc.pred_out || pl.Cout <= 32) && conv_takes_sb(m, pl, cc.stride, cc.decide_N > 0 ? cc.decide_N : cc.N, cc.Hs, cc.Ws))) {
        // split the input into three bf16 terms (SB16) unless its producer already wrote it that way, then the convolution
        // on the bf16 matrix cores; the small launches (a few frames of a small map) stay on the fp32 kernels
        Workspace& ws = const_cast<bde_model*>(m)->W();
        const bool grouped_in = cc.in_gs != 0;
        const long frames = (grouped_in ? pl.G : 1) * (long)cc.N;
        const long need = split_bf16_bytes(frames, pl.Cin, (long)cc.Hs * cc.Ws);
        if (cc.in_sb || (ws.sb && need <= ws.sb_bytes)) {
            if (!cc.in_sb) BDE_TRY(split_bf16(cc.in, ws.sb, frames, pl.Cin, (long)cc.Hs * cc.Ws, m->sb_terms, m->ovf(), s));
            ConvArgs b = a;
            b.in = cc.in_sb ? cc.in : ws.sb;
            b.wpk = m->P(pl.split_off(m->sb_terms));
            b.w_gs = pl.split_sz(m->sb_terms);
            b.acc_scale = m->P(pl.sh_unscale_off);
            b.nchunks = pl.sb_chunks;
            b.zeros = m->P(m->zero_off);
            b.in_ns = (long)pl.sb_chunks * cc.Hs * cc.Ws * sb_pix_bytes(m->sb_terms) / 4;
            b.in_gs = cc.in_sb ? cc.in_gs : (grouped_in ? b.in_ns * cc.N : 0);
            bool launched = false;
            BDE_TRY(conv_sb_launch(pl.KS, cc.stride, b, pl.G, s, &launched));
            pl.sb_used = launched ? 1 : 0;
            if (launched) return BDE_OK;
        }
        if (cc.in_sb) return fail(BDE_ERR_UNSUPPORTED, "convolution on a split-bf16 input has no split-bf16 launch at this size");
    }
    pl.sb_used = 0;
    return conv_launch_best(pl.KS, cc.stride, a, pl.G, s);
}

// The head ConvLayer (V5.py:116, submodules.py:105-114: 5x5, <= 5 bins -> basechannels, ReLU) of `N` voxel grids.  Where the packing
// has it (pack_head3) and the scratch image fits, on the three-columns-per-chunk image: split_head3_kernel + conv_sb_kernel<KS_HEAD3>,
// ten MFMA taps instead of twenty-five 16-channel chunks that are 11/16 zeros; otherwise the generic path (run_conv).
static int run_head_conv(const bde_model* m, const float* ev, float* out, int N, int H, int W, hipStream_t s) {
    const PackedLayer& pl = m->head;
    Workspace& ws = const_cast<bde_model*>(m)->W();
    const int ti = m->sb_terms - 2;
    const bool h3 = m->head3 && m->conv_sb && (ti == 0 || ti == 1) && pl.h3_off[ti] >= 0 && pl.Cout == 32 && pl.KS == 5 && H >= 16 && W >= 16 &&
                    (long)N * H * W >= 16384 && ws.sb != nullptr && (long)N * H * (W + 3) * sb_pix_bytes(m->sb_terms) <= ws.sb_bytes;
    if (h3) {
        BDE_TRY(split_head3(ev, ws.sb, N, pl.Cin, H, W, m->sb_terms, m->ovf(), s));
        ConvArgs a;
        memset(&a, 0, sizeof a);
        a.in = ws.sb;
        a.wpk = m->P(pl.h3_off[ti]);
        a.w_gs = pl.h3_sz[ti];
        a.bias = m->P(pl.b_off);
        a.bias_gs = pl.Cout;
        a.out = out;
        a.N = N;
        a.Cin = pl.Cin;
        a.Cout = pl.Cout;
        a.Hs = a.Hin = a.Ho = H;
        a.Ws = a.Win = W + 3;
        a.Wo = W;
        a.nchunks = 1;
        a.act = ACT_RELU;
        a.in_ns = (long)H * (W + 3) * sb_pix_bytes(m->sb_terms) / 4;
        a.out_ns = a.res1_ns = a.res2_ns = (long)pl.Cout * H * W;
        a.xcd_remap = m->xcd_remap;
        a.sb_terms = m->sb_terms;
        a.acc_scale = m->P(pl.sh_unscale_off);
        a.zeros = m->P(m->zero_off);
        bool launched = false;
        BDE_TRY(conv_sb_launch_head3(a, s, &launched));
        if (launched) {
            pl.sb_used = 1;
            return BDE_OK;
        }
    }
    ConvCall hc;
    hc.pl = &pl;
    hc.in = ev;
    hc.out = out;
    hc.N = N;
    hc.Hs = H;
    hc.Ws = W;
    hc.act = ACT_RELU;
    return run_conv(m, hc, s);
}

// 1x1 conv over flattened [C][HW] planes
static int run_pw(const bde_model* m, const PackedLayer* pl, const float* in, float* out, int N, long HW, int act,
                  const float* res1, const float* res2, int mask_w, int mask_pt, int mask_pl, hipStream_t s) {
    ConvCall cc;
    cc.pl = pl;
    cc.in = in;
    cc.out = out;
    cc.N = N;
    cc.Hs = 1;
    cc.Ws = (int)HW;
    cc.act = act;
    cc.res1 = res1;
    cc.res2 = res2;
    cc.mask_w = mask_w;
    cc.mask_pt = mask_pt;
    cc.mask_pl = mask_pl;
    return run_conv(m, cc, s);
}

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------
static int ws_alloc(Workspace& ws, float** p, long numel) {
    void* q = nullptr;
    BDE_HIP(hipMalloc(&q, sizeof(float) * (size_t)std::max<long>(numel, 4)));
    ws.allocs.push_back(q);
    *p = (float*)q;
    return BDE_OK;
}

static bool winblock_ok(const bde_model* m, int l);
static bool wide_ok(const bde_model* m, int l);
static bool split_chain_ok(const bde_model* m, int l);
static bool lstm_sb_ok(const bde_model* m, int l, int B, int h, int w);
static bool lstm_sbk_ok(const bde_model* m, int l, int h, int w);
static bool lstm_sbx_ok(const bde_model* m, int l, int h, int w);

static int ensure_workspace(bde_model* m, int T, int B, int H, int W) {
    Workspace& ws = m->W();
    if (ws.T == T && ws.B == B && ws.H == H && ws.W == W) return BDE_OK;
    ws.release();
    const bde_config& c = m->cfg;
    const int L = c.num_encoders;
    const long TB = (long)T * B;
    BDE_TRY(ws_alloc(ws, &ws.ev, TB * c.num_bins * H * W));
    BDE_TRY(ws_alloc(ws, &ws.head, TB * c.basechannels * H * W));
    BDE_TRY(ws_alloc(ws, &ws.out, TB * H * W));
    ws.xenc.assign(L, nullptr); ws.gx.assign(L, nullptr); ws.hseq.assign(L, nullptr); ws.cst.assign(L, nullptr);
    ws.hsb.assign(L, nullptr); ws.ghb.assign(L, nullptr); ws.hsk.assign(L, nullptr);
    ws.gur.assign(L, nullptr); ws.ghr.assign(L, nullptr); ws.gou.assign(L, nullptr); ws.gub.assign(L, nullptr);
    const bool gru = c.use_rc && c.recurrent_type == 1;
    ws.mergedS.assign(L, nullptr); ws.mstats.assign(L, nullptr);
    ws.merged.assign(L, nullptr); ws.mergedT.assign(L, nullptr); ws.kvun.assign(L, nullptr); ws.kvref.assign(L, nullptr); ws.dec.assign(L, nullptr); ws.qkv0.assign(L, nullptr);
    long max_attn = 0;
    for (int l = 0; l < L; ++l) {
        const long C = m->cout(l), hw = (long)(H >> (l + 1)) * (W >> (l + 1));
        const long hwp = cdivl(hw, 16) * 16;              // token tiles of 16 (wideblock.h)
        BDE_TRY(ws_alloc(ws, &ws.xenc[l], 2 * TB * C * hw));
        BDE_TRY(ws_alloc(ws, &ws.hseq[l], 2 * TB * C * hw));
        BDE_TRY(ws_alloc(ws, &ws.cst[l], 2 * (long)B * C * hw));
        if (gru) {
            BDE_TRY(ws_alloc(ws, &ws.gur[l], 2L * B * 2 * C * hw));
            BDE_TRY(ws_alloc(ws, &ws.ghr[l], 2L * B * C * hw));
            BDE_TRY(ws_alloc(ws, &ws.gou[l], 2L * B * C * hw));
            BDE_TRY(ws_alloc(ws, &ws.gub[l], 2L * B * C * hw));
        }
        if (!gru && c.use_rc && lstm_sbk_ok(m, l, H >> (l + 1), W >> (l + 1)))
            BDE_TRY(ws_alloc(ws, &ws.hsk[l], 2 * split_bf16_bytes(2L * B, (int)C, hw) / 4 + 4));
        // x-part of the gates of all frames, both directions -- the largest buffer of a level (20 GB at 480 x 640, T = 32, B = 4);
        // not needed where the recurrent step contracts [x | h] itself (lstm_fuse_x)
        if (!lstm_sbx_ok(m, l, H >> (l + 1), W >> (l + 1))) BDE_TRY(ws_alloc(ws, &ws.gx[l], 2 * TB * 4 * C * hw));
        if (!gru && c.use_rc && lstm_sb_ok(m, l, B, H >> (l + 1), W >> (l + 1))) {
            BDE_TRY(ws_alloc(ws, &ws.hsb[l], 2 * split_bf16_bytes(2L * B, (int)C, hw) / 4 + 4));
            BDE_TRY(ws_alloc(ws, &ws.ghb[l], 2L * B * 4 * C * hw));
        }
        BDE_TRY(ws_alloc(ws, &ws.merged[l], TB * C * hw));
        if (c.depths[l] > 0) {
            if (winblock_ok(m, l)) {
                // one-launch blocks recompute the neighbours' K|V: only the token-major twin of merged is staged
                // (the K|V stacks of the split path are 71 GB at 1280x720, T = 64)
                BDE_TRY(ws_alloc(ws, &ws.mergedT[l], TB * C * hw));
            } else if (wide_ok(m, l)) {
                // fragment-layout twin of merged (token tiles of 16) + token-major K|V stacks
                BDE_TRY(ws_alloc(ws, &ws.mergedT[l], TB * C * hwp));
                if (split_chain_ok(m, l)) {                    // ... and its SPL16 twin + statistics (wide_core.h)
                    BDE_TRY(ws_alloc(ws, &ws.mergedS[l], TB * C * hwp));
                    BDE_TRY(ws_alloc(ws, &ws.mstats[l], TB * hwp * 2));
                }
                BDE_TRY(ws_alloc(ws, &ws.kvun[l], TB * c.depths[l] * 2 * C * hw));
                BDE_TRY(ws_alloc(ws, &ws.kvref[l], TB * c.depths[l] * 2 * C * hw));
            } else {
                BDE_TRY(ws_alloc(ws, &ws.kvun[l], TB * c.depths[l] * 2 * C * hw));
                BDE_TRY(ws_alloc(ws, &ws.kvref[l], TB * c.depths[l] * 2 * C * hw));
                BDE_TRY(ws_alloc(ws, &ws.qkv0[l], TB * 3 * C * hw));
            }
            max_attn = std::max(max_attn, (long)B * C * hwp);
        }
        const int j = L - 1 - l;   // decoder j writes the map of level (L-1-j)'s input resolution
        BDE_TRY(ws_alloc(ws, &ws.dec[j], TB * m->cin(l) * (long)(H >> l) * (W >> l)));
    }
    BDE_TRY(ws_alloc(ws, &ws.up, TB * m->cout(0) * (long)H * W));   // dec L-1: cout(0) channels at full resolution
    if (c.skip_concat) {
        // largest cat(skip, x): decoder inputs 2 * cout(l) at level l, predI input 2 * basechannels at full resolution
        long mc = TB * 2 * c.basechannels * (long)H * W;
        for (int l = 0; l < L; ++l) mc = std::max(mc, TB * 2 * m->cout(l) * (long)(H >> (l + 1)) * (W >> (l + 1)));
        BDE_TRY(ws_alloc(ws, &ws.cat, mc));
        BDE_TRY(ws_alloc(ws, &ws.fuse, mc / 2));
    }
    if (c.depths[L - 1] == 0) {
        const long n = (long)B * m->cout(L - 1) * (long)(H >> L) * (W >> L);
        BDE_TRY(ws_alloc(ws, &ws.rbA, n));
        BDE_TRY(ws_alloc(ws, &ws.rbX[0], n));
        BDE_TRY(ws_alloc(ws, &ws.rbX[1], n));
        BDE_TRY(ws_alloc(ws, &ws.zero_l, n));
        BDE_HIP(hipMemset(ws.zero_l, 0, sizeof(float) * n));
    }
    {
        // split-bf16 image of one convolution's input (6 B per element, channels padded to 16): the largest of the
        // encoder inputs, gate-conv inputs (both directions) and upsampled decoder inputs
        long mx = 0;
        for (int l = 0; l < L; ++l) {
            const long hw_in = (long)(H >> l) * (W >> l), hw = (long)(H >> (l + 1)) * (W >> (l + 1));
            mx = std::max(mx, split_bf16_bytes(TB, m->cin(l), hw_in));               // encoder conv input
            mx = std::max(mx, split_bf16_bytes(2 * TB, m->cout(l), hw));             // gate conv input, both directions
            mx = std::max(mx, split_bf16_bytes(TB, m->cout(l), 4 * hw));             // decoder conv input (upsampled)
        }
        ws.sb_bytes = mx;
        BDE_TRY(ws_alloc(ws, &ws.sb, mx / 4 + 4));
        long mx2 = 0;
        for (int l = 0; l < L; ++l) mx2 = std::max(mx2, split_bf16_bytes(2 * TB, m->cout(l), (long)(H >> (l + 1)) * (W >> (l + 1))));
        ws.sb2_bytes = mx2;
        BDE_TRY(ws_alloc(ws, &ws.sb2, mx2 / 4 + 4));
    }
    if (max_attn > 0) {
        BDE_TRY(ws_alloc(ws, &ws.qkv, 3 * max_attn));
        BDE_TRY(ws_alloc(ws, &ws.ao, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.x1, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.hid, 4 * max_attn));
        BDE_TRY(ws_alloc(ws, &ws.xa, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.xb, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.xaS, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.xbS, max_attn));
        BDE_TRY(ws_alloc(ws, &ws.stA, max_attn / 64 + 64));       // (two floats per token of at least 128 channels)
        BDE_TRY(ws_alloc(ws, &ws.stB, max_attn / 64 + 64));
        float* cnt = nullptr;                              // one counter per 16 tokens of the largest attention frame
        BDE_TRY(ws_alloc(ws, &cnt, max_attn / 16 + 64));
        BDE_HIP(hipMemset(cnt, 0, sizeof(int) * (size_t)(max_attn / 16 + 64)));
        ws.tile_count = reinterpret_cast<int*>(cnt);
    }
    ws.T = T; ws.B = B; ws.H = H; ws.W = W;
    return BDE_OK;
}

// ------------------------------------------------------------------------------------------
// stages
// ------------------------------------------------------------------------------------------
// RecurrentConv sweep of one level for both directions (V5.py:122-135; submodules.py:191-195).
//   in: [TB][Cin][H][W].  Results: ws.hseq[l] = [2][TB][C][h][w]; ws.cst[l] final cell states.
// dir_mask: bit0 forward, bit1 backward (the op-level test runs a single direction).
// Non-recurrent part of a level for frames [f0, f0+nf) of the [TB] stack: encoder conv (both
// directions read the same sequence, V5.py:124-130) and the x-part of the gates.
static int run_enc_gx(bde_model* m, int l, const float* in, int f0, int nf, int T, int B, int H, int W, hipStream_t s) {
    Workspace& ws = m->W();
    const int Cin = m->cin(l), C = m->cout(l), h = H / 2, w = W / 2;
    const long TB = (long)T * B, hw = (long)h * w;
    // one direction only (bde_split_sweep): one-group views of the layers, pointers moved to that direction's half
    const int dmask = m->dir_mask, dsel = dmask == 2 ? 1 : 0;
    const bool one_dir = dmask != 3;
    const PackedLayer enc_v = one_dir ? group_view(m->enc[l], dsel) : m->enc[l];
    const PackedLayer gx_v = (one_dir && m->cfg.use_rc) ? group_view(m->gx[l], dsel) : m->gx[l];
    ConvCall e;
    e.pl = &enc_v;
    e.in = in + (long)f0 * Cin * H * W;
    e.out = ws.xenc[l] + (long)f0 * C * hw;
    e.N = nf;
    e.Hs = H;
    e.Ws = W;
    e.stride = 2;
    e.act = ACT_RELU;
    e.in_gs = 0;
    e.out_gs = TB * C * hw;
    if (!m->cfg.use_rc) {
        // bare ConvLayer encoders (V5.py:256-258): the convolution's output IS the level's feature sequence
        e.out = ws.hseq[l] + (long)f0 * C * hw + (one_dir ? dsel * e.out_gs : 0);
        ProfScope ps(m, pname("enc_conv", l), s);
        const int st = run_conv(m, e, s);
        m->enc[l].sb_used = enc_v.sb_used;
        return st;
    }
    if (one_dir) e.out += dsel * e.out_gs;
    // the gate convolution reads its input as SB16 (conv_sb.h): the encoder conv's epilogue then writes that image directly
    // (6 B per element) and the fp32 planes + their conversion pass are skipped
    const long sb_fs = (long)cdiv(C, 16) * hw * sb_pix_bytes(m->sb_terms) / 4;   // floats of one SB16 frame
    // (lstm_fuse_x: the recurrent step contracts [x | h] itself and reads x from that image: no gate convolution at all)
    const bool step_x = lstm_sbx_ok(m, l, h, w);
    const bool fuse = (step_x || (m->fuse_enc_sb && C % 32 == 0 && conv_takes_sb(m, gx_v, 1, nf, h, w))) &&
                      ws.sb2 && split_bf16_bytes(2 * TB, C, hw) <= ws.sb2_bytes;
    BDE_REQUIRE(fuse || !step_x, "recurrent step with the x-part: no room for the split image of x");
    if (fuse) {
        e.out_sb = ws.sb2 + (long)f0 * sb_fs + (one_dir ? dsel * TB * sb_fs : 0);
        e.out_sb_gs = TB * sb_fs;
    }
    { ProfScope ps(m, pname("enc_conv", l), s); BDE_TRY(run_conv(m, e, s)); }
    m->enc[l].sb_used = enc_v.sb_used;                                   // (the launch ran on a copy / one-direction view of the layer)
    if (step_x) { m->gx[l].sb_used = 0; return BDE_OK; }
    // gx = conv3x3(x; W[:, :C]) + bias   (submodules.py:316-317, x half of the stacked input)
    BDE_REQUIRE(ws.gx[l] != nullptr, "gate convolution: no x-part buffer at level %d", l);
    ConvCall gxc;
    gxc.pl = &gx_v;
    gxc.in = ws.xenc[l] + (long)f0 * C * hw + (one_dir ? dsel * TB * C * hw : 0);
    gxc.out = ws.gx[l] + (long)f0 * m->gx[l].Cout * hw + (one_dir ? dsel * TB * 4 * C * hw : 0);   // rows: 4C (ConvLSTM gates) or 3C (ConvGRU)
    gxc.N = nf;
    gxc.Hs = h;
    gxc.Ws = w;
    gxc.in_gs = TB * C * hw;
    gxc.out_gs = TB * 4 * C * hw;
    if (fuse) {
        gxc.in = ws.sb2 + (long)f0 * sb_fs + (one_dir ? dsel * TB * sb_fs : 0);
        gxc.in_gs = TB * sb_fs;
        gxc.in_sb = true;
    }
    { ProfScope ps(m, pname("gates_x", l), s); BDE_TRY(run_conv(m, gxc, s)); }
    m->gx[l].sb_used = gx_v.sb_used;
    return BDE_OK;
}

// The recurrent step on the bf16 matrix cores: h-part of the gates by conv_sb_kernel on the SB16 image of h_prev, then the
// pointwise tail as an element-wise kernel that also writes the next step's SB16 h.  Built, parity-tested
// (set_tuning("lstm_sb", 1)) and measured at the canonical config: a step is one small launch (368 / 176 / 96 workgroups at
// levels 0 / 1 / 2), each workgroup walks its 4 / 8 / 16 channel chunks with the halo staging exposed (one or two
// workgroups per CU; two LDS buffers leave a single workgroup per CU and two rounds at level 0): 69 us of convolution +
// 16.5 us of pointwise kernel per step against 65 us for lstm16_step_kernel.  Off by default.
static bool lstm_sb_ok(const bde_model* m, int l, int B, int h, int w) {
    if (m->lstm_sb_mode == 0 || !m->conv_sb) return false;
    const int C = m->cout(l);
    if (m->lstm_sb_off(l) < 0 || !conv_sb_fits(3, 1, 4 * C, w, h, w, m->sb_terms)) return false;
    if (m->lstm_sb_mode == 1) return true;
    const long wgs = cdivl((long)h * w, 128) * cdivl(4 * C, 128) * 2 * B;
    return wgs >= 160 && cdiv(C, 16) <= 8;
}

// The fused split-bf16 step (lstm_sb.h): one launch per time step, h carried as SB16 between steps (two buffers).
static bool lstm_sbk_ok(const bde_model* m, int l, int h, int w) {
    if (!m->use_lstm_sbk || m->lstm_sb_mode != 0 || !m->conv_sb) return false;
    if ((size_t)l >= m->lstm_sbk.size() || m->lstm_sbk[l].sb_off < 0) return false;
    return lstm_sb_shape(m->cout(l), h, w, m->sb_terms).ok;
}

// ... with the x-part of the gates in the same contraction: the encoder convolution of the level leaves x as an SB16 image
// (its epilogue writes it, any kernel), 32 | C so that whole 32-channel tiles are written
static bool lstm_sbx_ok(const bde_model* m, int l, int h, int w) {
    if (!m->lstm_fuse_x || !lstm_sbk_ok(m, l, h, w)) return false;
    const Workspace& ws = const_cast<bde_model*>(m)->W();
    if ((size_t)l >= ws.hsk.size() || ws.hsk[l] == nullptr) return false;      // the step that will run is not the split one
    return (size_t)l < m->lstm_sbx.size() && m->lstm_sbx[l].split_off(m->sb_terms) >= 0 && m->cout(l) % 32 == 0;
}

static int run_recurrent_steps_sbk(bde_model* m, int l, int T, int B, int h, int w, hipStream_t s) {
    Workspace& ws = m->W();
    const int C = m->cout(l);
    const long TB = (long)T * B, hw = (long)h * w;
    const bool step_x = lstm_sbx_ok(m, l, h, w);
    const PackedLayer& pl = step_x ? m->lstm_sbx[l] : m->lstm_sbk[l];
    float* hs = ws.hseq[l];
    const long dstride = TB * C * hw, fs = (long)B * C * hw;
    const int terms = m->sb_terms;
    const long sb_ns = (long)cdiv(C, 16) * hw * sb_pix_bytes(terms);       // bytes of one frame's SB16 image
    const long sb_buf = 2L * B * sb_ns;                                    // one buffer: both directions
    const int dsel = m->dir_mask == 2 ? 1 : 0;
    const bool one_dir = m->dir_mask != 3;
    unsigned char* hsk = reinterpret_cast<unsigned char*>(ws.hsk[l]);
    for (int st = 0; st < T; ++st) {
        const int tf = st, tb = T - 1 - st;
        ProfScope ps(m, pname("lstm", l), s);
        LstmSbArgs a;
        memset(&a, 0, sizeof a);
        a.hin = hsk + ((st + 1) & 1) * sb_buf;
        a.hsb = hsk + (st & 1) * sb_buf;
        a.hin_gs = (long)B * sb_ns;
        a.hin_ns = sb_ns;
        a.terms = terms;
        a.acc_scale = m->P(pl.sh_unscale_off);
        a.wpk = reinterpret_cast<const unsigned short*>(m->P(pl.split_off(terms)));
        a.w_gs = pl.split_sz(terms) * 2;
        if (!step_x) {
            BDE_REQUIRE(ws.gx[l] != nullptr, "recurrent step: no x-part buffer at level %d", l);
            a.gx = ws.gx[l] + (long)tf * B * 4 * C * hw;
            a.gx_gs = (ws.gx[l] + TB * 4 * C * hw + (long)tb * B * 4 * C * hw) - a.gx;
            a.gx_ns = (long)4 * C * hw;
        } else {
            // x_t of both directions in ws.sb2 (run_enc_gx): [direction][TB frames], forward reads frame tf, backward frame tb
            const unsigned char* xs = reinterpret_cast<const unsigned char*>(ws.sb2);
            a.xin = xs + (long)tf * B * sb_ns;
            a.xin_gs = (TB + (long)tb * B - (long)tf * B) * sb_ns;
            a.xin_ns = sb_ns;
            a.xchunks = C / 16;
            a.bias = m->P(pl.b_off);
        }
        a.cstate = ws.cst[l];
        a.c_gs = (long)B * C * hw;
        a.c_ns = (long)C * hw;
        a.hout = hs + (long)tf * fs;
        a.ho_gs = (hs + dstride + (long)tb * fs) - a.hout;
        a.ho_ns = (long)C * hw;
        a.zeros = m->P(m->zero_off);
        a.B = B; a.Ch = C; a.H = h; a.W = w;
        a.first = st == 0;
        a.stamps = (st == T / 2) ? m->tok_stamps : nullptr;                // diagnostics (bde_debug_token_stamps): one mid-sweep step
        a.stamp_mode = m->tok_debug == 9 ? 1 : 0;
        if (one_dir) {                                                     // group 0 of a one-group launch = the chosen direction
            a.hin += dsel * a.hin_gs; a.hsb += dsel * a.hin_gs;
            a.wpk += dsel * a.w_gs;
            if (step_x) { a.xin += dsel * a.xin_gs; a.bias += (long)dsel * 4 * C; }
            a.gx += dsel * a.gx_gs;
            a.cstate += dsel * a.c_gs;
            a.hout += dsel * a.ho_gs;
        }
        BDE_TRY(lstm_sb_step_launch(a, one_dir ? 1 : 2, s));
    }
    return BDE_OK;
}

static int run_recurrent_steps_sb(bde_model* m, int l, int T, int B, int h, int w, hipStream_t s) {
    Workspace& ws = m->W();
    const int C = m->cout(l);
    const long TB = (long)T * B, hw = (long)h * w;
    const PackedLayer& pl = m->lstm_sb[l];
    float* hs = ws.hseq[l];
    const long dstride = TB * C * hw, fs = (long)B * C * hw;
    const int terms = m->sb_terms;
    const long sbf = split_bf16_bytes(2L * B, C, hw, terms) / 4;   // floats of one SB16 hidden-state buffer (both directions)
    for (int st = 0; st < T; ++st) {
        const int tf = st, tb = T - 1 - st;
        ProfScope ps(m, pname("lstm", l), s);
        float* hsb_prev = ws.hsb[l] + ((st + 1) & 1) * sbf;
        float* hsb_next = ws.hsb[l] + (st & 1) * sbf;
        if (st > 0) {
            ConvArgs a;
            memset(&a, 0, sizeof a);
            a.in = hsb_prev;
            a.in_ns = (long)pl.sb_chunks * hw * sb_pix_bytes(terms) / 4;
            a.in_gs = a.in_ns * B;
            a.sb_terms = terms;
            a.acc_scale = m->P(pl.sh_unscale_off);
            a.wpk = m->P(pl.split_off(terms));
            a.w_gs = pl.split_sz(terms);
            a.bias = m->P(m->zero_off_long());                       // the gates' bias rides in gx
            a.bias_gs = 0;
            a.out = ws.ghb[l];
            a.out_ns = (long)4 * C * hw;
            a.out_gs = a.out_ns * B;
            a.res1_ns = a.res2_ns = a.out_ns;
            a.N = B; a.Cin = C; a.Hin = a.Hs = h; a.Win = a.Ws = w; a.Cout = 4 * C; a.Ho = h; a.Wo = w;
            a.nchunks = pl.sb_chunks;
            a.act = ACT_NONE;
            a.zeros = m->P(m->zero_off);
            bool launched = false;
            BDE_TRY(conv_sb_launch(3, 1, a, 2, s, &launched));
            BDE_REQUIRE(launched, "recurrent step: the split-bf16 convolution does not fit %dx%d", h, w);
        }
        LstmPointArgs p;
        memset(&p, 0, sizeof p);
        p.gx = ws.gx[l] + (long)tf * B * 4 * C * hw;
        p.gx_gs = (ws.gx[l] + TB * 4 * C * hw + (long)tb * B * 4 * C * hw) - p.gx;
        p.gx_ns = (long)4 * C * hw;
        p.gh = st > 0 ? ws.ghb[l] : nullptr;
        p.cstate = ws.cst[l];
        p.hout = hs + (long)tf * fs;
        p.h_gs = (hs + dstride + (long)tb * fs) - p.hout;
        p.h_ns = (long)C * hw;
        p.hsb = reinterpret_cast<unsigned short*>(hsb_next);
        p.C = C; p.B = B; p.HW = hw;
        p.first = st == 0;
        p.terms = terms;
        BDE_TRY(lstm_point_launch(p, s));
    }
    return BDE_OK;
}

// ConvGRU sweep of a level, both directions per launch (submodules.py:358-376; RecurrentConv.forward :191-195 returns the
// state itself).  Per step: h-parts of update | reset (one 3x3 convolution, 2C rows), gates + h * reset, h-part of the
// candidate on h * reset, blend.  The x-parts sit in ws.gx[l] as [2][TB][3C][hw] (update | reset | out).
static int run_gru_steps(bde_model* m, int l, int T, int B, int h, int w, hipStream_t s) {
    Workspace& ws = m->W();
    const int C = m->cout(l);
    const long TB = (long)T * B, hw = (long)h * w;
    float* hs = ws.hseq[l];
    const long dstride = TB * C * hw, fs = (long)B * C * hw;
    const int dsel = m->dir_mask == 2 ? 1 : 0;
    const bool one_dir = m->dir_mask != 3;
    const int G = one_dir ? 1 : 2;
    const PackedLayer ur_v = one_dir ? group_view(m->gru_ur[l], dsel) : m->gru_ur[l];
    const PackedLayer o_v = one_dir ? group_view(m->gru_o[l], dsel) : m->gru_o[l];
    const long total = (long)G * B * C * hw;
    const unsigned blocks = (unsigned)std::min<long>(cdivl(total, 256), 4096);
    for (int st = 0; st < T; ++st) {
        const int tf = st, tb = T - 1 - st;
        ProfScope ps(m, pname("gru", l), s);
        const float* hprev_f = hs + (long)(tf - 1) * fs;
        const float* hprev_b = hs + dstride + (long)(tb + 1) * fs;
        GruArgs g;
        memset(&g, 0, sizeof g);
        g.gx = ws.gx[l] + (long)tf * B * 3 * C * hw;
        g.gx_gs = (ws.gx[l] + TB * 4 * C * hw + (long)tb * B * 3 * C * hw) - g.gx;
        g.gx_ns = 3L * C * hw;
        g.ubuf = ws.gub[l];
        g.hr = ws.ghr[l];
        g.hout = hs + (long)tf * fs;
        g.ho_gs = (hs + dstride + (long)tb * fs) - g.hout;
        g.ho_ns = (long)C * hw;
        g.C = C; g.B = B; g.HW = hw; g.G = G;
        if (one_dir) {                                                 // group 0 of the launches = the chosen direction
            g.gx += dsel * g.gx_gs;
            g.hout += dsel * g.ho_gs;
        }
        if (st > 0) {
            g.hprev = one_dir && dsel ? hprev_b : hprev_f;
            g.hp_gs = hprev_b - hprev_f;
            g.hp_ns = (long)C * hw;
            ConvCall ur;
            ur.pl = &ur_v;
            ur.in = g.hprev; ur.in_gs = hprev_b - hprev_f;
            ur.out = ws.gur[l]; ur.out_gs = (long)B * 2 * C * hw;
            ur.N = B; ur.Hs = h; ur.Ws = w;
            BDE_TRY(run_conv(m, ur, s));
            g.gh_ur = ws.gur[l];
        }
        hipLaunchKernelGGL(gru_gate_kernel, dim3(blocks), dim3(256), 0, s, g);
        if (st > 0) {
            ConvCall oc;
            oc.pl = &o_v;
            oc.in = ws.ghr[l]; oc.in_gs = (long)B * C * hw;
            oc.out = ws.gou[l]; oc.out_gs = (long)B * C * hw;
            oc.N = B; oc.Hs = h; oc.Ws = w;
            BDE_TRY(run_conv(m, oc, s));
            g.gh_o = ws.gou[l];
        }
        hipLaunchKernelGGL(gru_out_kernel, dim3(blocks), dim3(256), 0, s, g);
        BDE_HIP(hipGetLastError());
    }
    return BDE_OK;
}

static int run_recurrent_level(bde_model* m, int l, const float* in, int T, int B, int H, int W, hipStream_t s,
                               bool enc_done = false) {
    Workspace& ws = m->W();
    const int C = m->cout(l), h = H / 2, w = W / 2;
    const long TB = (long)T * B, hw = (long)h * w;
    if (!enc_done && !(m->debug_skip & 16)) BDE_TRY(run_enc_gx(m, l, in, 0, (int)TB, T, B, H, W, s));
    if (!m->cfg.use_rc) return BDE_OK;
    if (m->cfg.recurrent_type == 1) return run_gru_steps(m, l, T, B, h, w, s);
    if ((size_t)l < m->lstm_sbk.size()) m->lstm_sbk[l].sb_used = ws.hsk[l] != nullptr ? 1 : 0;
    if (!(m->debug_skip & 4) && ws.hsk[l] != nullptr) {
        if (m->lstm_two_streams && m->dir_mask == 3 && !m->prof_on) {
            // A step launch's workgroups run in lockstep: prologue, halo wait and the pointwise tail (a quarter of the cycles)
            // leave the matrix cores idle chip-wide.  The forward and the backward sweep are independent until the merge
            // (V5.py:122-147): as two chains of one-direction launches on two streams they drift apart and one direction's
            // MFMA phases cover the other's tails.  Same launches per direction as bde_split_sweep: results are bit-identical.
            const int slot = m->cur;
            if (!m->dir_stream[slot]) {
                BDE_HIP(hipStreamCreateWithFlags(&m->dir_stream[slot], hipStreamNonBlocking));
                BDE_HIP(hipEventCreateWithFlags(&m->dir_fork[slot], hipEventDisableTiming));
                BDE_HIP(hipEventCreateWithFlags(&m->dir_join[slot], hipEventDisableTiming));
            }
            hipStream_t s2 = m->dir_stream[slot];
            BDE_HIP(hipEventRecord(m->dir_fork[slot], s));
            BDE_HIP(hipStreamWaitEvent(s2, m->dir_fork[slot], 0));
            m->dir_mask = 1;
            int st = run_recurrent_steps_sbk(m, l, T, B, h, w, s);
            m->dir_mask = 2;
            if (st == BDE_OK) st = run_recurrent_steps_sbk(m, l, T, B, h, w, s2);
            m->dir_mask = 3;
            BDE_HIP(hipEventRecord(m->dir_join[slot], s2));
            BDE_HIP(hipStreamWaitEvent(s, m->dir_join[slot], 0));
            return st;
        }
        return run_recurrent_steps_sbk(m, l, T, B, h, w, s);
    }
    if (!(m->debug_skip & 4) && ws.hsb[l] != nullptr) {
        BDE_REQUIRE(m->dir_mask == 3, "the split-bf16 recurrent step (lstm_sb) runs both directions only");
        return run_recurrent_steps_sb(m, l, T, B, h, w, s);
    }
    // T recurrent steps; group 0 = forward at t = s, group 1 = backward at t = T-1-s
    const int dsel = m->dir_mask == 2 ? 1 : 0;
    const bool one_dir = m->dir_mask != 3;
    const PackedLayer& pl = m->lstm[l];
    float* hs = ws.hseq[l];
    const long dstride = TB * C * hw;          // direction stride inside hseq
    const long fs = (long)B * C * hw;          // one time step (B frames)
    for (int st = 0; st < T && !(m->debug_skip & 4); ++st) {
        const int tf = st, tb = T - 1 - st;
        ConvArgs a;
        memset(&a, 0, sizeof a);
        a.first = (st == 0);
        const float* hprev_f = hs + (long)(tf - 1) * fs;               // unused when first
        const float* hprev_b = hs + dstride + (long)(tb + 1) * fs;
        if (a.first) { hprev_f = hs; hprev_b = hs; }
        a.in = hprev_f;
        a.in_gs = hprev_b - hprev_f;
        a.in_ns = (long)C * hw;
        a.wpk = m->P(pl.w_off);
        a.w_gs = pl.w_sz;
        a.bias = m->P(pl.b_off);
        a.out = hs + (long)tf * fs;
        a.out_gs = (hs + dstride + (long)tb * fs) - a.out;
        a.out_ns = (long)C * hw;
        a.gx = ws.gx[l] + (long)tf * B * 4 * C * hw;
        a.gx_gs = (ws.gx[l] + TB * 4 * C * hw + (long)tb * B * 4 * C * hw) - a.gx;
        a.gx_ns = (long)4 * C * hw;
        a.cstate = ws.cst[l];
        a.c_gs = (long)B * C * hw;
        a.c_ns = (long)C * hw;
        if (one_dir) {                                                 // group 0 of a one-group launch = the chosen direction
            a.lstm_groups = 1;
            a.in += dsel * a.in_gs;
            a.wpk += dsel * a.w_gs;
            a.bias += (long)dsel * 4 * C;
            a.out += dsel * a.out_gs;
            a.gx += dsel * a.gx_gs;
            a.cstate += dsel * a.c_gs;
        }
        a.N = B;
        a.Cin = C;
        a.Hin = a.Hs = h;
        a.Win = a.Ws = w;
        a.Cout = 4 * C;
        a.Ho = h;
        a.Wo = w;
        a.nchunks = pl.nchunks;
        {
            ProfScope ps(m, pname("lstm", l), s);
            const bool hc8 = m->lstm_hc8 == 1 || (m->lstm_hc8 < 0 && lstm16_wants_hc8(a));
            if (hc8) {                                   // 8-channel workgroups: their own weight packing
                a.w_gs = m->lstm8[l].w_sz;
                a.wpk = m->P(m->lstm8[l].w_off) + (one_dir ? dsel * a.w_gs : 0);
            }
            BDE_TRY(lstm16_launch(a, s, hc8));
        }
    }
    return BDE_OK;
}

// DFrameAttention + in-place refinement for one target frame (V5.py:154-169; DTransformer.py:376-389).
//   xq      : query frame [B][C][HW] (slot q_idx)
//   kvslot  : per slot, base of the [B][depth*2C][HW] K|V stack of that frame (nullptr = zero frame);
//             ignored for slot q_idx
//   addres  : tensor added to the result (merged[t], V5.py:166) or nullptr
//   out     : [B][C][HW]
//   qkv_first: q|k|v of block blk0 for xq if already computed (batched over T), else nullptr
static int run_attention_frame(bde_model* m, int l, const float* xq, const float* const* kvslot, const float* addres,
                               float* out, int B, int H, int W, int blk0, int nblk, const float* qkv_first,
                               hipStream_t s) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const AttnLevel& al = m->attn[l];
    const int C = al.C, D = c.frame_num;
    const long HW = (long)H * W;
    const int ph = (7 - H % 7) % 7, pw = (7 - W % 7) % 7;   // DTransformer.py:260-263
    const int pt = ph / 2, plft = pw / 2;
    const int Hp = H + ph, Wp = W + pw;
    const float* x = xq;
    const bool fused = al.blocks[0].proj16 >= 0 && cdivl(HW, 32) * B >= m->fused_min_tiles;
    bool have_qkv = false;                                   // the fused kernel leaves the next block's q|k|v in ws.qkv
    for (int i = blk0; i < blk0 + nblk; ++i) {
        const AttnBlock& ab = al.blocks[i];
        const bool dil = (i % 2) == 1;                       // DTransformer.py:362
        const bool last = (i == blk0 + nblk - 1);
        // q | k | v of the current x
        const float* qkv = ws.qkv;
        if (i == blk0 && qkv_first) qkv = qkv_first;
        else if (!have_qkv) { ProfScope ps(m, pname("chain_qkv", l), s); BDE_TRY(run_pw(m, &ab.qkv, x, ws.qkv, B, HW, ACT_NONE, nullptr, nullptr, 0, 0, 0, s)); }
        AttnArgs a;
        memset(&a, 0, sizeof a);
        a.q = qkv;
        a.q_bs = 3 * C * HW;
        for (int d = 0; d < D; ++d) {
            if (d == c.q_idx) {
                a.kv[d] = qkv + (long)C * HW;
                a.kv_bs[d] = 3 * C * HW;
            } else if (kvslot[d]) {
                a.kv[d] = kvslot[d] + (long)i * 2 * C * HW;
                a.kv_bs[d] = (long)al.depth * 2 * C * HW;
            } else {
                a.kv[d] = nullptr;
            }
            a.v_off[d] = (long)C * HW;
        }
        a.kvpad = m->P(ab.kvpad_off);
        a.biasT = m->P(ab.bias_off);
        a.out = ws.ao;
        a.out_bs = C * HW;
        a.D = D; a.C = C; a.heads = c.num_heads; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp;
        a.pt = pt; a.pl = plft; a.nWw = Wp / 7; a.dilated = dil ? 1 : 0;
        {
            ProfScope ps(m, pname("chain_core", l), s);
            BDE_TRY(attn_launch(a, B, s));
        }
        float* dst = last ? out : (x == ws.xa ? ws.xb : ws.xa);
        if (fused) {
            TokenArgs ta;
            memset(&ta, 0, sizeof ta);
            ta.ao = ws.ao;
            ta.x = x;
            ta.addres = last ? addres : nullptr;
            ta.x2 = dst;
            ta.wproj = m->P(ab.proj16);  ta.bproj = m->P(ab.proj.b_off);
            ta.wfc1 = m->P(ab.fc1_16);   ta.bfc1 = m->P(ab.fc1.b_off);  ta.sfc1 = m->P(ab.fc1.s_off);
            ta.wfc2 = m->P(ab.fc2_16);   ta.bfc2 = m->P(ab.fc2.b_off);
            if (!last) {
                const AttnBlock& nb = al.blocks[i + 1];
                ta.qkv = ws.qkv;
                ta.wqkv = m->P(nb.qkv16);  ta.bqkv = m->P(nb.qkv.b_off);  ta.sqkv = m->P(nb.qkv.s_off);
            }
            ta.bs_c = (long)C * HW;
            ta.bs_qkv = 3L * C * HW;
            ta.C = C;
            ta.HW = (int)HW;
            ta.mask_w = dil ? W : 0;
            ta.mask_pt = pt;
            ta.mask_pl = plft;
            ta.debug = m->tok_debug;
            ta.stamps = m->tok_stamps;
            { ProfScope ps(m, pname("chain_token", l), s); BDE_TRY(token_launch(ta, B, s)); }
            have_qkv = !last;
            x = dst;
            continue;
        }
        // x1 = shortcut + proj(attn)   (uncovered pixels of a dilated block: shortcut only)
        { ProfScope ps(m, pname("chain_proj", l), s); BDE_TRY(run_pw(m, &ab.proj, ws.ao, ws.x1, B, HW, ACT_NONE, x, nullptr, dil ? W : 0, pt, plft, s)); }
        // x2 = x1 + fc2(GELU(fc1(LN(x1))))  (+ merged[t] after the last block)
        { ProfScope ps(m, pname("chain_mlp_in", l), s); BDE_TRY(run_pw(m, &ab.fc1, ws.x1, ws.hid, B, HW, ACT_GELU, nullptr, nullptr, 0, 0, 0, s)); }
        { ProfScope ps(m, pname("chain_mlp_out", l), s); BDE_TRY(run_pw(m, &ab.fc2, ws.hid, dst, B, HW, ACT_NONE, ws.x1, last ? addres : nullptr, 0, 0, 0, s)); }
        x = dst;
    }
    return BDE_OK;
}

static bool winblock_ok(const bde_model* m, int l) {
    const AttnLevel& al = m->attn[l];
    return m->winblock && al.depth > 0 && al.blocks[0].biasF_off >= 0 && al.blocks[0].qkv16 >= 0;
}

// One frame through the blocks of a level with winblock.h.  Everything is token-major [B][HW][C]:
//   frames[d]: frame of slot d (nullptr = zero frame), frames[q_idx] = the query frame
//   addres   : added to the result (merged[t], V5.py:166) or nullptr
//   out_tok  : result, token-major;  out_nchw: the same result as [B][C][HW] planes (may be nullptr)
static int run_attention_frame_win(bde_model* m, int l, const float* const* frames, const float* addres, float* out_tok,
                                   float* out_nchw, int B, int H, int W, int blk0, int nblk, hipStream_t s) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const AttnLevel& al = m->attn[l];
    const int C = al.C, D = c.frame_num;
    const long HW = (long)H * W;
    const int ph = (7 - H % 7) % 7, pw = (7 - W % 7) % 7;   // DTransformer.py:260-263
    const float* x = frames[c.q_idx];
    for (int i = blk0; i < blk0 + nblk; ++i) {
        const AttnBlock& ab = al.blocks[i];
        const bool last = (i == blk0 + nblk - 1);
        float* dst = last ? out_tok : (x == ws.xa ? ws.xb : ws.xa);
        WinArgs a;
        memset(&a, 0, sizeof a);
        a.slot[0] = x;
        a.slot_bs[0] = C * HW;
        int k = 1;
        for (int d = 0; d < D; ++d) {
            if (d == c.q_idx) continue;
            a.slot[k] = frames[d];
            a.slot_bs[k] = C * HW;
            ++k;
        }
        a.nslots = D;
        a.addres = last ? addres : nullptr;
        a.addres_bs = C * HW;
        a.out = dst;
        a.out_nchw = last ? out_nchw : nullptr;
        a.out_bs = C * HW;
        a.wqkv = m->P(ab.qkv16);   a.bqkv = m->P(ab.qkv.b_off);  a.sqkv = m->P(ab.qkv.s_off);
        a.wproj = m->P(ab.proj16); a.bproj = m->P(ab.proj.b_off);
        a.wfc1 = m->P(ab.fc1_16);  a.bfc1 = m->P(ab.fc1.b_off);  a.sfc1 = m->P(ab.fc1.s_off);
        a.wfc2 = m->P(ab.fc2_16);  a.bfc2 = m->P(ab.fc2.b_off);
        a.biasF = m->P(ab.biasF_off);
        const bool sbk = m->winblock_sb && ab.qkvS >= 0;
        if (sbk) {
            const bool two = m->sb_terms == 2;
            a.terms = two ? 2 : 3;
            a.wqkvS = reinterpret_cast<const unsigned short*>(m->P(two ? ab.qkvH : ab.qkvS));
            a.wprojS = reinterpret_cast<const unsigned short*>(m->P(two ? ab.projH : ab.projS));
            a.wfc1S = reinterpret_cast<const unsigned short*>(m->P(two ? ab.fc1H : ab.fc1S));
            a.wfc2S = reinterpret_cast<const unsigned short*>(m->P(two ? ab.fc2H : ab.fc2S));
            a.unscale = m->P(ab.unscaleH);
            a.ovf = m->ovf();
        }
        a.stamps = m->tok_stamps;
        a.H = H; a.W = W; a.Hp = H + ph; a.Wp = W + pw; a.pt = ph / 2; a.pl = pw / 2;
        a.dilated = (i % 2) == 1 ? 1 : 0;                    // DTransformer.py:362
        { ProfScope ps(m, pname("winblock", l), s); BDE_TRY(sbk ? winblock_sb_launch(a, B, s) : winblock_launch(a, B, s)); }
        x = dst;
    }
    return BDE_OK;
}

static bool wide_ok(const bde_model* m, int l) {
    const AttnLevel& al = m->attn[l];
    return al.depth > 0 && !winblock_ok(m, l) && al.kvallW >= 0 && al.blocks[0].qkvW >= 0 &&
           m->cfg.frame_num * ATT_TOK <= 160;
}

// The split chain of a wide level (wideblock.h, wide_core.h, wide_mlp.h; bde_model::wide_kv_sb): two-term operands, C = 256,
// head_dim 16, every pack present.  Otherwise a wide level runs the fp32 chain.
static bool split_chain_ok(const bde_model* m, int l) {
    const AttnLevel& al = m->attn[l];
    if (!(m->wide_kv_sb && m->wide_fuse_mlp && m->sb_terms == 2 && al.C == 256 && m->cfg.num_heads * 16 == al.C && al.depth > 0 &&
          al.kvallH >= 0))
        return false;
    for (const AttnBlock& ab : al.blocks)
        if (ab.biasW_off < 0 || ab.qkvN < 0 || ab.projHF < 0 || ab.fc1N < 0 || ab.fc2N < 0 || ab.fc1.Cout != 4 * al.C) return false;
    return true;
}

// One GEMM of the wide chain (wideblock.h): x FRAG16 [B][ntile][K/16][256] -> token-major or FRAG16
static int run_tokgemm(bde_model* m, const char* span, int l, long w_off, const PackedLayer& pl, int M, int K, const float* x, int B,
                       long HW, float* out_tok, float* out_frag, int act, const float* res, const float* addres, float* out_nchw,
                       int mask_w, int mask_pt, int mask_pl, hipStream_t s, long wH_off = -1, long wH_unscale = -1) {
    TokGemmArgs a;
    memset(&a, 0, sizeof a);
    const int ntile = (int)cdivl(HW, 16);
    a.x = x;
    a.w = m->P(w_off);
    a.bias = m->P(pl.b_off);
    a.lnsum = pl.s_off >= 0 ? m->P(pl.s_off) : nullptr;
    a.out_tok = out_tok;
    a.out_frag = out_frag;
    a.out_nchw = out_nchw;
    a.res = res;
    a.addres = addres;
    a.x_bs = (long)ntile * 16 * K;
    a.out_bs = out_tok ? HW * M : (long)ntile * 16 * M;
    a.res_bs = a.addres_bs = (long)ntile * 16 * M;
    a.nchw_bs = HW * M;
    a.K = K; a.M = M; a.HW = (int)HW; a.ntile = ntile;
    a.act = act;
    a.mask_w = mask_w; a.mask_pt = mask_pt; a.mask_pl = mask_pl;
    ProfScope ps(m, pname(span, l), s);
    if (wH_off >= 0 && split_chain_ok(m, l)) {          // the split chain's K|V: two fp16 terms on the matrix cores (tokgemm_sb_*kernel)
        a.wS = reinterpret_cast<const unsigned short*>(m->P(wH_off));
        a.w_unscale = m->P(wH_unscale);
        a.ovf = m->ovf();
        if (tokgemm_sb_fits(a)) return tokgemm_sb_launch(a, B, s);
    }
    return tokgemm_launch(a, B, s);
}

// DFrameAttention + refinement for one target frame on the wide chain.  Everything FRAG16 / token-major:
//   xq       : query frame, FRAG16 [B][ntile][C/16][256]
//   kvslot[d]: token-major K|V stack [B][HW][depth*2C] of slot d's frame (nullptr = zero frame; ignored for q_idx)
//   addres   : FRAG16 tensor added to the result (merged[t]) or nullptr;   out: FRAG16;   out_nchw: optional [B][C][HW]
//   prev_frag / prev_slot: FRAG16 frame of ONE refined neighbour (buffer slot prev_slot) whose K | V the attention core computes
//              itself (wide_core.h) instead of reading kvslot[prev_slot]; nullptr = none (split chain only)
//   xq_twin / prev_twin: SPL16 twins of xq / prev_frag; out_twin: where the last block writes the twin of out (split chain only)
struct WideTwin { float* s = nullptr; float* st = nullptr; };     // SPL16 image (as float*) and statistics of a FRAG16 frame, or nothing
static int run_attention_frame_wide(bde_model* m, int l, const float* xq, const float* const* kvslot, const float* addres, float* out,
                                    float* out_nchw, int B, int H, int W, int blk0, int nblk, hipStream_t s,
                                    const float* prev_frag = nullptr, int prev_slot = -1, WideTwin xq_twin = WideTwin(),
                                    WideTwin out_twin = WideTwin(), WideTwin prev_twin = WideTwin()) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const AttnLevel& al = m->attn[l];
    const int C = al.C, D = c.frame_num;
    const long HW = (long)H * W;
    const int ph = (7 - H % 7) % 7, pw = (7 - W % 7) % 7;   // DTransformer.py:260-263
    const int pt = ph / 2, plft = pw / 2;
    const int ntile = (int)cdivl(HW, 16);
    const float* x = xq;
    if (split_chain_ok(m, l)) {
        // split chain: every frame the core reads has its SPL16 twin, and every block writes the twin of its output (mlp_fused_kernel)
        BDE_REQUIRE(xq_twin.s && out_twin.s && (!prev_frag || prev_twin.s) && ws.tile_count,
                    "wide split chain: SPL16 twins of the frames are missing");
        WideTwin xt = xq_twin;
        for (int i = blk0; i < blk0 + nblk; ++i) {
            const AttnBlock& ab = al.blocks[i];
            const bool dil = (i % 2) == 1;                   // DTransformer.py:362
            const bool last = (i == blk0 + nblk - 1);
            WideCoreArgs a;
            memset(&a, 0, sizeof a);
            a.x_bs = (long)ntile * 16 * C;
            a.q_slot = c.q_idx;
            a.p_slot = prev_frag ? prev_slot : -1;
            for (int d = 0; d < D; ++d) {
                a.kv[d] = nullptr;
                if (d == c.q_idx || (prev_frag && d == prev_slot) || !kvslot[d]) continue;
                a.kv[d] = kvslot[d]; a.kv_bs[d] = HW * al.depth * 2 * C; a.kv_ld[d] = al.depth * 2 * C;
                a.k_off[d] = i * 2 * C; a.v_off[d] = i * 2 * C + C;
            }
            a.kvpad = m->P(ab.kvpad_off);
            a.biasW = m->P(ab.biasW_off);
            a.wqkvS = reinterpret_cast<const unsigned short*>(m->P(ab.qkvN));
            a.wqkv_unscale = m->P(ab.qkvN_unscale);
            a.xS = reinterpret_cast<const unsigned short*>(xt.s);
            a.xSt = xt.st;
            a.xpS = prev_frag ? reinterpret_cast<const unsigned short*>(prev_twin.s) : nullptr;
            a.xpSt = prev_frag ? prev_twin.st : nullptr;
            a.spl_bs = (long)ntile * 16 * C * 2;             // 16-bit elements: two terms per value
            a.st_bs = (long)ntile * 16 * 2;
            a.zeros = m->P(m->zero_off);
            a.bqkv = m->P(ab.qkv.b_off);
            a.sqkv = m->P(ab.qkv.s_off);
            a.out = ws.ao;
            a.D = D; a.C = C; a.heads = c.num_heads; a.H = H; a.W = W; a.Hp = H + ph; a.Wp = W + pw;
            a.pt = pt; a.pl = plft; a.nWw = (W + pw) / 7; a.dilated = dil ? 1 : 0; a.ntile = ntile;
            a.stamps = m->tok_debug == 22 ? m->tok_stamps : nullptr;
            { ProfScope ps(m, pname("wide_core", l), s); BDE_TRY(wide_core_launch(a, B, s)); }
            // x2 = x1 + fc2(GELU(fc1(LN(x1)))), x1 = shortcut + proj(attn): the whole token half of the block in one launch (wide_mlp.h)
            float* dst = (last && out) ? out : (x == ws.xa ? ws.xb : ws.xa);     // out == nullptr: the caller only wants out_nchw
            const WideTwin dt = last ? out_twin : (dst == ws.xa ? WideTwin{ws.xaS, ws.stA} : WideTwin{ws.xbS, ws.stB});
            MlpFusedArgs fa;
            memset(&fa, 0, sizeof fa);
            fa.ao = ws.ao; fa.x = x;
            fa.wprojS = reinterpret_cast<const unsigned short*>(m->P(ab.projHF));
            fa.wfc1S = reinterpret_cast<const unsigned short*>(m->P(ab.fc1N));
            fa.wfc2S = reinterpret_cast<const unsigned short*>(m->P(ab.fc2N));
            fa.unscale_proj = m->P(ab.projHF_unscale);
            fa.unscale_mlp = m->P(ab.mlpN_unscale);
            fa.bproj = m->P(ab.proj.b_off);
            fa.bfc1 = m->P(ab.fc1.b_off);
            fa.sfc1 = m->P(ab.fc1.s_off);
            fa.bfc2 = m->P(ab.fc2.b_off);
            fa.part = ws.hid;                                // (the hidden activations never leave the workgroups)
            fa.count = ws.tile_count;
            fa.out = dst;
            fa.out_nchw = last ? out_nchw : nullptr;
            fa.addres = last ? addres : nullptr;
            fa.x_bs = (long)ntile * 16 * C;
            fa.nchw_bs = HW * C;
            fa.HW = (int)HW; fa.ntile = ntile; fa.B = B;
            fa.mask_w = dil ? W : 0; fa.mask_pt = pt; fa.mask_pl = plft;
            fa.ovf = m->ovf();
            fa.out_spl = reinterpret_cast<unsigned short*>(dt.s);
            fa.out_stats = dt.st;
            fa.spl_bs = (long)ntile * 16 * C * 2;
            fa.st_bs = (long)ntile * 16 * 2;
            fa.stamps = m->tok_debug == 21 ? m->tok_stamps : nullptr;
            { ProfScope ps(m, pname("wide_mlp", l), s); BDE_TRY(mlp_fused_launch(fa, s)); }
            x = dst;
            xt = dt;
        }
        return BDE_OK;
    }
    // fp32 chain
    BDE_REQUIRE(prev_frag == nullptr, "wide fp32 chain: K | V of the refined frame are expected in kvslot");
    for (int i = blk0; i < blk0 + nblk; ++i) {
        const AttnBlock& ab = al.blocks[i];
        const bool dil = (i % 2) == 1;                       // DTransformer.py:362
        const bool last = (i == blk0 + nblk - 1);
        AttnTokArgs a;
        memset(&a, 0, sizeof a);
        a.x = x;                                             // q | k | v of the query frame inside the attention core (wideblock.h)
        a.x_bs = (long)ntile * 16 * C;
        a.wqkv = m->P(ab.qkvW);
        a.bqkv = m->P(ab.qkv.b_off);
        a.sqkv = m->P(ab.qkv.s_off);
        a.q_slot = c.q_idx;
        for (int d = 0; d < D; ++d) {
            a.kv[d] = nullptr;
            if (d == c.q_idx || !kvslot[d]) continue;
            a.kv[d] = kvslot[d]; a.kv_bs[d] = HW * al.depth * 2 * C; a.kv_ld[d] = al.depth * 2 * C;
            a.k_off[d] = i * 2 * C; a.v_off[d] = i * 2 * C + C;
        }
        a.kvpad = m->P(ab.kvpad_off);
        a.biasT = m->P(ab.bias_off);
        a.out = ws.ao;
        a.out_bs = (long)ntile * 16 * C;
        a.D = D; a.C = C; a.heads = c.num_heads; a.H = H; a.W = W; a.Hp = H + ph; a.Wp = W + pw;
        a.pt = pt; a.pl = plft; a.nWw = (W + pw) / 7; a.dilated = dil ? 1 : 0; a.ntile = ntile;
        { ProfScope ps(m, pname("wide_core", l), s); BDE_TRY(attn_tok16_launch(a, B, s)); }
        float* dst = (last && out) ? out : (x == ws.xa ? ws.xb : ws.xa);     // out == nullptr: the caller only wants out_nchw
        // x1 = shortcut + proj(attn)   (uncovered pixels of a dilated block: shortcut only; DTransformer.py:299, 79-82)
        BDE_TRY(run_tokgemm(m, "wide_proj", l, ab.projW, ab.proj, C, C, ws.ao, B, HW, nullptr, ws.x1, ACT_NONE, x, nullptr, nullptr,
                            dil ? W : 0, pt, plft, s));
        // x2 = x1 + fc2(GELU(fc1(LN(x1))))  (+ merged[t] after the last block; DTransformer.py:279-283,304, V5.py:166)
        BDE_TRY(run_tokgemm(m, "wide_mlp_in", l, ab.fc1W, ab.fc1, 4 * C, C, ws.x1, B, HW, nullptr, ws.hid, ACT_GELU, nullptr, nullptr,
                            nullptr, 0, 0, 0, s));
        BDE_TRY(run_tokgemm(m, "wide_mlp_out", l, ab.fc2W, ab.fc2, C, 4 * C, ws.hid, B, HW, nullptr, dst, ACT_NONE, ws.x1,
                            last ? addres : nullptr, last ? out_nchw : nullptr, 0, 0, 0, s));
        x = dst;
    }
    return BDE_OK;
}

typedef int (*FrameDoneFn)(bde_model* m, int t, void* ctx);
static int run_attention_level(bde_model* m, int l, int T, int B, int H, int W, hipStream_t s,
                               FrameDoneFn on_frame = nullptr, void* ctx = nullptr) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const AttnLevel& al = m->attn[l];
    const int C = al.C, D = c.frame_num;
    const long HW = (long)H * W, fs = (long)B * C * HW;
    const long kvfs = (long)B * al.depth * 2 * C * HW;
    if (winblock_ok(m, l)) {
        // one launch per block; the K|V of the neighbour frames are recomputed inside from the frames
        // themselves (refined in place for f < t, V5.py:166-169), so nothing else is staged per level
        { ProfScope ps(m, pname("to_tok", l), s); BDE_TRY(nchw_to_tok(ws.merged[l], ws.mergedT[l], T * B, C, (int)HW, s)); }
        for (int t = 0; t < T; ++t) {
            const float* frames[BDE_MAX_FRAMES];
            for (int d = 0; d < D; ++d) {
                const int f = t + c.buffer_index[d];
                frames[d] = (f < 0 || f >= T) ? nullptr : ws.mergedT[l] + (long)f * fs;
            }
            float* mt = ws.mergedT[l] + (long)t * fs;
            frames[c.q_idx] = mt;
            BDE_TRY(run_attention_frame_win(m, l, frames, mt, mt, ws.merged[l] + (long)t * fs, B, H, W, 0, al.depth, s));
            if (on_frame) BDE_TRY(on_frame(m, t, ctx));
        }
        return BDE_OK;
    }
    bool need_un = false, need_ref = false;
    for (int d = 0; d < D; ++d) {
        if (d == c.q_idx) continue;
        if (c.buffer_index[d] >= 0) need_un = true; else need_ref = true;
    }
    if (wide_ok(m, l)) {
        const int ntile = (int)cdivl(HW, 16);
        const long ffs = (long)B * ntile * 16 * C;           // FRAG16 frame stride
        const bool twins = split_chain_ok(m, l);
        BDE_REQUIRE(!twins || ws.mergedS[l], "wide split chain: the workspace has no SPL16 twins");
        const long sfs = ffs, stfs = (long)B * ntile * 16 * 2;    // SPL16 frame stride (floats of the image) / statistics stride
        {
            ProfScope ps(m, pname("to_frag", l), s);
            if (twins) BDE_TRY(nchw_to_frag_spl(ws.merged[l], ws.mergedT[l], reinterpret_cast<unsigned short*>(ws.mergedS[l]), ws.mstats[l], T * B,
                                                C, (int)HW, m->ovf(), s));
            else BDE_TRY(nchw_to_frag(ws.merged[l], ws.mergedT[l], T * B, C, (int)HW, s));
        }
        if (need_un)
            BDE_TRY(run_tokgemm(m, "wide_kv_all", l, al.kvallW, al.kvall, al.depth * 2 * C, C, ws.mergedT[l], T * B, HW, ws.kvun[l],
                                nullptr, ACT_NONE, nullptr, nullptr, nullptr, 0, 0, 0, s, al.kvallH, al.kvallH_unscale));
        // one refined neighbour (one negative buffer offset): its K | V are computed by the attention core of the frame that reads
        // them (wide_core.h), from the neighbour's refined FRAG16 frame -- no K|V GEMM between two frames of the chain
        int nneg = 0, neg_slot = -1;
        for (int d = 0; d < D; ++d)
            if (d != c.q_idx && c.buffer_index[d] < 0) { ++nneg; neg_slot = d; }
        const bool in_core = twins && nneg == 1;
        for (int t = 0; t < T; ++t) {
            const float* kvslot[BDE_MAX_FRAMES];
            const float* prev_frag = nullptr;
            WideTwin qt, pt;
            if (twins) qt = WideTwin{ws.mergedS[l] + (long)t * sfs, ws.mstats[l] + (long)t * stfs};
            for (int d = 0; d < D; ++d) {
                const int f = t + c.buffer_index[d];
                if (d == c.q_idx || f < 0 || f >= T) kvslot[d] = nullptr;
                else if (f < t && in_core) {
                    kvslot[d] = nullptr;
                    prev_frag = ws.mergedT[l] + (long)f * ffs;
                    if (twins) pt = WideTwin{ws.mergedS[l] + (long)f * sfs, ws.mstats[l] + (long)f * stfs};
                }
                else if (f < t) kvslot[d] = ws.kvref[l] + (long)f * kvfs;      // refined (V5.py:166-169)
                else kvslot[d] = ws.kvun[l] + (long)f * kvfs;
            }
            float* mtF = ws.mergedT[l] + (long)t * ffs;
            BDE_TRY(run_attention_frame_wide(m, l, mtF, kvslot, mtF, mtF, ws.merged[l] + (long)t * fs, B, H, W, 0, al.depth, s,
                                             prev_frag, neg_slot, qt, qt, pt));
            if (need_ref && !in_core && t + 1 < T)
                BDE_TRY(run_tokgemm(m, "wide_kv", l, al.kvallW, al.kvall, al.depth * 2 * C, C, mtF, B, HW, ws.kvref[l] + (long)t * kvfs,
                                    nullptr, ACT_NONE, nullptr, nullptr, nullptr, 0, 0, 0, s, al.kvallH, al.kvallH_unscale));
            if (on_frame) BDE_TRY(on_frame(m, t, ctx));
        }
        return BDE_OK;
    }
    // K|V of every block for the still-unrefined frames, all T at once
    if (need_un) {
        ProfScope ps(m, pname("chain_kv_all", l), s);
        BDE_TRY(run_pw(m, &al.kvall, ws.merged[l], ws.kvun[l], T * B, HW, ACT_NONE, nullptr, nullptr, 0, 0, 0, s));
    }
    // q|k|v of the first block for every frame at once: its input is the still-unrefined merged[t]
    { ProfScope ps(m, pname("chain_qkv_all", l), s); BDE_TRY(run_pw(m, &al.blocks[0].qkv, ws.merged[l], ws.qkv0[l], T * B, HW, ACT_NONE, nullptr, nullptr, 0, 0, 0, s)); }
    for (int t = 0; t < T; ++t) {
        const float* kvslot[BDE_MAX_FRAMES];
        for (int d = 0; d < D; ++d) {
            const int f = t + c.buffer_index[d];
            if (d == c.q_idx || f < 0 || f >= T) kvslot[d] = nullptr;
            else if (f < t) kvslot[d] = ws.kvref[l] + (long)f * kvfs;      // refined (V5.py:166-169)
            else kvslot[d] = ws.kvun[l] + (long)f * kvfs;
        }
        float* mt = ws.merged[l] + (long)t * fs;
        BDE_TRY(run_attention_frame(m, l, mt, kvslot, mt, mt, B, H, W, 0, al.depth, ws.qkv0[l] + (long)t * B * 3 * C * HW, s));
        if (need_ref && t + 1 < T) {
            ProfScope ps(m, pname("chain_kv", l), s);
            BDE_TRY(run_pw(m, &al.kvall, mt, ws.kvref[l] + (long)t * kvfs, B, HW, ACT_NONE, nullptr, nullptr, 0, 0, 0, s));
        }
        if (on_frame) BDE_TRY(on_frame(m, t, ctx));
    }
    return BDE_OK;
}

// UpsampleConvLayer of decoder j on N frames [Cin][Hs][Ws] (+ skip): upsample kernel, then a plain conv.
// predI + the output activation ride in the conv's epilogue when one workgroup holds every output channel of a pixel
// (Cout <= 64: the 32 channels of the canonical last decoder are one MFMA row tile)
static bool pred_fusable(const bde_model* m) { return m->cfg.basechannels <= 64 && m->fuse_pred && !m->cfg.skip_concat; }

// skip_concat in front of a decoder or of predI (V5.py:285-286, 86-93): y = Conv1x1(cat(first, second)) on N frames of
// [C][hw] each -> ws.fuse
static int run_concat_fuse(bde_model* m, const PackedLayer& pl, const float* first, const float* second, int N, int C, long hw,
                           hipStream_t s) {
    Workspace& ws = m->W();
    BDE_TRY(concat_channels(first, second, ws.cat, N, (long)C * hw, (long)C * hw, s));
    return run_pw(m, &pl, ws.cat, ws.fuse, N, hw, ACT_NONE, nullptr, nullptr, 0, 0, 0, s);
}

// The last level without attention (depths[-1] == 0): Sequential(ParseLayer, ResidualBlockNoBN x n) on the frame buffer
// (V5.py:77-80, 151-169).  ParseLayer takes buffer SLOT 0 (:281-282), i.e. the frame at offset buffer_index[0] -- refined
// already when that offset is negative, still unrefined when it is not, zeros outside the sequence -- and the result is added
// to merged[t] in place: sequential in t like the attention.
static int run_bottleneck_level(bde_model* m, int l, int T, int B, int h, int w, hipStream_t s) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const int C = m->cout(l), nb = c.num_res_blocks;
    const long fs = (long)B * C * h * w;
    for (int t = 0; t < T; ++t) {
        ProfScope ps(m, pname("bottleneck", l), s);
        const int f = t + c.buffer_index[0];
        float* mt = ws.merged[l] + (long)t * fs;
        const float* x = (f < 0 || f >= T) ? ws.zero_l : ws.merged[l] + (long)f * fs;
        if (nb == 0) { BDE_TRY(add2(x, mt, mt, fs, s)); continue; }
        for (int k = 0; k < nb; ++k) {
            ConvCall c1;                                     // relu(conv1(x))
            c1.pl = &m->rb1[k]; c1.in = x; c1.out = ws.rbA; c1.N = B; c1.Hs = h; c1.Ws = w; c1.act = ACT_RELU;
            BDE_TRY(run_conv(m, c1, s));
            const bool last = k == nb - 1;
            ConvCall c2;                                     // x + conv2(.)   (+ merged[t] after the last block, V5.py:166)
            c2.pl = &m->rb2[k]; c2.in = ws.rbA; c2.N = B; c2.Hs = h; c2.Ws = w; c2.act = ACT_NONE;
            c2.res1 = x;
            c2.res2 = last ? mt : nullptr;
            c2.out = last ? mt : ws.rbX[k & 1];
            BDE_TRY(run_conv(m, c2, s));
            x = c2.out;
        }
    }
    return BDE_OK;
}

// Parts of a forward (forward_on): PART_PRE = head and the first level's encoder convolution, PART_MAIN = everything between it and
// the last kernel that writes split operands (the captured graph), PART_TAIL = what follows that kernel -- the last decoder
// convolution (+ predI) of the frames decoded last.  The overflow word of the range guard (split.h) is read back in front of the
// tail, so the host learns about an overflow while the tail still runs; PART_ALL = the whole forward in one piece.
enum { PART_ALL = 0, PART_MAIN = 1, PART_TAIL = 2, PART_PRE = 3 };

static int run_decoder(bde_model* m, int j, const float* in, const float* skip, float* out, int N, int Hs, int Ws,
                       hipStream_t s, const float* pred_head = nullptr, float* pred_out = nullptr, int part = PART_ALL, int decide_N = 0) {
    const PackedLayer& pl = m->dec[j];
    Workspace& ws = m->W();
    if (decide_N <= 0) decide_N = N;
    // a split-bf16 convolution reads SB16: the upsampling kernel then writes that image directly (no fp32 map, no conversion)
    const bool to_sb = m->fuse_enc_sb && (!pred_out || pl.Cout <= 32) && conv_takes_sb(m, pl, 1, decide_N, 2 * Hs, 2 * Ws) && ws.sb &&
                       split_bf16_bytes(N, pl.Cin, 4L * Hs * Ws) <= ws.sb_bytes;
    if (part != PART_TAIL) {
        ProfScope ps(m, pname("dec_up", j), s);
        if (to_sb) BDE_TRY(upsample2x_sum_split(in, skip, ws.sb, N, pl.Cin, Hs, Ws, m->sb_terms, m->ovf(), s));
        else BDE_TRY(upsample2x_sum(in, skip, ws.up, Hs, Ws, (long)N * pl.Cin, s));
    }
    if (part == PART_MAIN) return BDE_OK;
    ConvCall d;
    d.pl = &pl;
    d.in = to_sb ? ws.sb : ws.up;
    d.in_sb = to_sb;
    d.out = out;
    d.N = N;
    d.Hs = 2 * Hs;
    d.Ws = 2 * Ws;
    d.act = ACT_RELU6;
    d.pred_head = pred_head;
    d.pred_out = pred_out;
    d.decide_N = decide_N;
    ProfScope ps(m, pname("dec_conv", j), s);
    return run_conv(m, d, s);
}

static int check_dims(const bde_model* m, int T, int B, int H, int W) {
    const bde_config& c = m->cfg;
    BDE_REQUIRE(m->finalized, "weights are not finalized");
    BDE_REQUIRE(T >= 1 && B >= 1, "T=%d B=%d", T, B);
    const int mult = 1 << c.num_encoders;
    BDE_REQUIRE(H > 0 && W > 0 && H % mult == 0 && W % mult == 0, "H=%d W=%d must be multiples of %d", H, W, mult);
    for (int l = 0; l < c.num_encoders; ++l)
        if (c.depths[l] > 0)
            BDE_REQUIRE((H >> (l + 1)) >= 7 && (W >> (l + 1)) >= 7,
                        "feature map %dx%d at attention level %d is smaller than the 7x7 window (the reference "
                        "raises there too)", H >> (l + 1), W >> (l + 1), l);
    return BDE_OK;
}

static int forward_on(bde_model* m, const float* const* events, int T, int B, int H, int W, float* const* images,
                      hipStream_t s);

// The internal streams of the pipelined mode live as long as the process (one set per device, shared by the models
// on it): the caller's allocator may hold them as the last user of a tensor (record_stream) long after a model is
// gone, and recording on a destroyed stream faults.
static int pipeline_stream(int slot, hipStream_t* out) {
    static hipStream_t pool[BDE_MAX_DEVICES][bde_model::MAX_SLOTS] = {};
    int d = 0;
    BDE_HIP(hipGetDevice(&d));
    BDE_REQUIRE(d >= 0 && d < BDE_MAX_DEVICES, "device %d", d);
    if (!pool[d][slot]) BDE_HIP(hipStreamCreateWithFlags(&pool[d][slot], hipStreamNonBlocking));
    *out = pool[d][slot];
    return BDE_OK;
}

// ---- range guard of the two-term operand format: host side (split.h; bde_model::ovf_dev) ---------------------------------------
// Copy the current slot's overflow word to its pinned mirror and mark the point with the slot's event (forward_on).
static int note_overflow_readback(bde_model* m, hipStream_t s) {
    bde_model::Pending& p = m->pend[m->cur];
    if (!p.done) BDE_HIP(hipEventCreateWithFlags(&p.done, hipEventDisableTiming));
    BDE_HIP(hipMemcpyAsync(m->ovf_host + m->cur, m->ovf_dev + m->cur, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    BDE_HIP(hipEventRecord(p.done, s));
    return BDE_OK;
}
// Remember what a forward needs to be recomputed: its stream, shape and output pointers (its events stay in the workspace).
static void note_pending(bde_model* m, int slot, hipStream_t s, int T, int B, int H, int W, float* const* images) {
    bde_model::Pending& p = m->pend[slot];
    p.on = true; p.stream = s; p.T = T; p.B = B; p.H = H; p.W = W;
    p.images.assign(images, images + T);
}
// Look at the overflow words of all forwards issued so far (waits for them).  None set: nothing to do.  Otherwise, "sb_auto" = 1:
// the model switches to three bf16 terms for good and the forwards that overflowed are recomputed from the events their
// workspaces still hold, into the same output buffers, on the streams they ran on; "sb_auto" = 0: BDE_ERR_RANGE.
static int settle_overflow(bde_model* m) {
    bool flagged[bde_model::MAX_SLOTS] = {};
    int nflag = 0;
    for (int i = 0; i < bde_model::MAX_SLOTS; ++i) {
        bde_model::Pending& p = m->pend[i];
        if (!p.on) continue;
        BDE_HIP(hipEventSynchronize(p.done));
        if (m->ovf_host[i] != 0) { flagged[i] = true; ++nflag; }
    }
    if (nflag == 0) {
        for (auto& p : m->pend) p.on = false;
        return BDE_OK;
    }
    m->sb_overflows += nflag;
    for (int i = 0; i < bde_model::MAX_SLOTS; ++i) m->ovf_host[i] = 0;
    if (!m->sb_auto) {
        for (auto& p : m->pend) p.on = false;
        return fail(BDE_ERR_RANGE, "%d forward(s): an activation reached 65520, beyond the two fp16 terms of the default operand format "
                    "(csrc/split.h); the frames of those calls are not valid.  set_tuning(\"sb_terms\", 3) or \"sb_auto\" = 1", nflag);
    }
    // every forward issued so far has to be complete before the workspaces go (the switch of formats releases them)
    for (int i = 0; i < bde_model::MAX_SLOTS; ++i)
        if (m->pend[i].on) BDE_HIP(hipStreamSynchronize(m->pend[i].stream));
    struct Redo { int slot; float* ev; long ev_fs; };
    std::vector<Redo> redo;
    for (int i = 0; i < bde_model::MAX_SLOTS; ++i) {
        if (!flagged[i]) continue;
        const bde_model::Pending& p = m->pend[i];
        const long ev_fs = (long)p.B * m->cfg.num_bins * p.H * p.W;
        float* ev = nullptr;
        BDE_HIP(hipMalloc((void**)&ev, sizeof(float) * ev_fs * p.T));
        BDE_HIP(hipMemcpy(ev, m->wslots[i].ev, sizeof(float) * ev_fs * p.T, hipMemcpyDeviceToDevice));
        redo.push_back({i, ev, ev_fs});
    }
    for (auto& w : m->wslots) w.release();
    m->sb_terms = 3;
    m->sb_latched = 1;
    int st = BDE_OK;
    for (const Redo& r : redo) {
        bde_model::Pending p = m->pend[r.slot];
        std::vector<const float*> evp(p.T);
        for (int t = 0; t < p.T; ++t) evp[t] = r.ev + (long)t * r.ev_fs;
        m->cur = r.slot;
        if (st == BDE_OK) st = forward_on(m, evp.data(), p.T, p.B, p.H, p.W, p.images.data(), p.stream);
        (void)hipStreamSynchronize(p.stream);
        (void)hipFree(r.ev);
    }
    m->cur = 0;
    for (auto& p : m->pend) p.on = false;
    return st;
}

// Pipelined dispatch: call i runs on internal stream i%depth with workspace i%depth.  Inputs are ordered
// after the caller's stream by an event; outputs are ordered back by bde_wait_outputs (or by the
// next call that reuses the slot).
static int forward_impl(bde_model* m, const float* const* events, int T, int B, int H, int W, float* const* images,
                        hipStream_t user) {
    if (m->pipeline < 2) {
        // (a forward still pending here was issued in pipelined mode: look at it before its slot's word is reused)
        for (const auto& p : m->pend) if (p.on) { BDE_TRY(settle_overflow(m)); break; }
        m->cur = 0;
        BDE_TRY(forward_on(m, events, T, B, H, W, images, user));
        if (m->ovf() == nullptr) return BDE_OK;
        // default mode: the frames are final when this call returns, so the overflow word is looked at here -- the host waits
        // for the forward up to its last operand split while the tail (the last convolution) is still running
        note_pending(m, 0, user, T, B, H, W, images);
        return settle_overflow(m);
    }
    const int slot = (int)(m->ncalls++ % m->pipeline);
    if (m->pend[slot].on) BDE_TRY(settle_overflow(m));       // the slot's previous forward must be final before its workspace is reused
    if (!m->pstream[slot]) {
        BDE_TRY(pipeline_stream(slot, &m->pstream[slot]));
        BDE_HIP(hipEventCreateWithFlags(&m->pin[slot], hipEventDisableTiming));
        BDE_HIP(hipEventCreateWithFlags(&m->pout[slot], hipEventDisableTiming));
    }
    m->cur = slot;
    BDE_HIP(hipEventRecord(m->pin[slot], user));
    BDE_HIP(hipStreamWaitEvent(m->pstream[slot], m->pin[slot], 0));
    m->last_stream = m->pstream[slot];
    const int st = forward_on(m, events, T, B, H, W, images, m->pstream[slot]);
    if (st == BDE_OK && m->ovf() != nullptr) note_pending(m, slot, m->pstream[slot], T, B, H, W, images);
    BDE_HIP(hipEventRecord(m->pout[slot], m->pstream[slot]));
    m->pbusy[slot] = true;
    m->cur = 0;
    return st;
}

// Everything between the input copy and the output copy: pointers depend only on the workspace,
// so the launch sequence can be captured once per (slot, T, B, H, W) into a hipGraph and replayed
// (~630 launches per forward at config A; replay removes their host cost).
static int forward_body(bde_model* m, int T, int B, int H, int W, hipStream_t s, int part);
static bool side_decode_on(const bde_model* m, int T);

static int forward_on(bde_model* m, const float* const* events, int T, int B, int H, int W, float* const* images,
                      hipStream_t s) {
    BDE_TRY(check_dims(m, T, B, H, W));
    BDE_TRY(ensure_workspace(m, T, B, H, W));
    Workspace& ws = m->W();
    const long ev_fs = (long)B * m->cfg.num_bins * H * W, img_fs = (long)B * H * W;
    BDE_TRY(copy_frames(events, ws.ev, T, ev_fs, 0, s));
    ProfScope whole(m, "forward", s);
    // Range guard (split.h): the slot's overflow word starts at zero and is read back behind the last kernel that writes split
    // operands -- in front of the forward's tail where the tail is a launch of its own (no side-stream decode, the upsampling
    // kernel writes the last convolution's operand image itself), behind it otherwise.
    // In the default mode (one sequence in flight) the host waits for that word before bde_forward returns: the forward is then
    // cut in three -- head + first encoder convolution launched eagerly (PART_PRE: the chip has work while the host replays the
    // graph), the graph (PART_MAIN), the last convolution launched eagerly behind the read-back (PART_TAIL).
    const bool guard = m->ovf() != nullptr;
    const bool cut = guard && m->eager_cut && m->pipeline < 2 && m->fuse_enc_sb && !(m->debug_skip & (8 | 16)) && !m->prof_on;
    const int part_main = cut ? PART_MAIN : PART_ALL;
    if (guard) BDE_HIP(hipMemsetAsync(m->ovf(), 0, sizeof(unsigned), s));
    if (cut) BDE_TRY(forward_body(m, T, B, H, W, s, PART_PRE));
    // (profiling spans are captured as event-record nodes).  A schedule with a forked decode ("overlap") runs eagerly: a second
    // instantiated graph with a forked branch crashed inside hipGraphLaunch on its first launch, its own side stream and events
    // notwithstanding, while the first one replayed
    const bool can_graph = m->use_graph && ws.warm && !side_decode_on(m, T);
    if (ws.graph_exec && ws.graph_part != part_main) { (void)hipGraphExecDestroy(ws.graph_exec); ws.graph_exec = nullptr; }
    if (can_graph && !ws.graph_exec) {
        // capture on a private stream (the caller's may be the legacy default stream, which cannot
        // capture); the instantiated graph is then launched on the caller's stream
        if (!m->cap_stream) BDE_HIP(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        BDE_HIP(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
        const int st = forward_body(m, T, B, H, W, m->cap_stream, part_main);
        ws.graph_part = part_main;
        const hipError_t e = hipStreamEndCapture(m->cap_stream, &graph);
        hipError_t ei = hipSuccess;
        if (st == BDE_OK && e == hipSuccess) ei = hipGraphInstantiate(&ws.graph_exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (st != BDE_OK || e != hipSuccess || ei != hipSuccess) {
            // capture is an optimisation: fall back to eager launches for good
            (void)hipGetLastError();
            ws.graph_exec = nullptr;
            m->use_graph = 0;
        }
    }
    if (m->use_graph && can_graph && ws.graph_exec) {
        BDE_HIP(hipGraphLaunch(ws.graph_exec, s));
    } else {
        BDE_TRY(forward_body(m, T, B, H, W, s, part_main));
        ws.warm = true;                       // first call of a shape runs eagerly (one-time kernel attribute setup)
    }
    if (guard && cut) BDE_TRY(note_overflow_readback(m, s));
    if (cut) BDE_TRY(forward_body(m, T, B, H, W, s, PART_TAIL));     // one or two launches: not worth a graph of their own
    if (guard && !cut) BDE_TRY(note_overflow_readback(m, s));
    BDE_TRY(copy_frames(images, ws.out, T, img_fs, 1, s));
    return BDE_OK;
}

// C. decoder for frames [f0, f0 + nf) of the [T*B] stack (V5.py:183-197)
static int decode_frames(bde_model* mm, int f0, int nf, int T_, int B_, int H_, int W_, hipStream_t st, int part = PART_ALL) {
    // C. decoder (V5.py:183-197): x = L[-1]; x = dec_j(L[-1-j] + x); img = act(predI(x + head))
    Workspace& w = mm->W();
    const int L_ = mm->L;
    const float* x = w.merged[L_ - 1] + (long)f0 * mm->cout(L_ - 1) * (H_ >> L_) * (W_ >> L_);
    for (int j = 0; j < L_; ++j) {
        const int l = L_ - 1 - j;
        const long in_fs = (long)mm->cout(l) * (H_ >> (l + 1)) * (W_ >> (l + 1));
        const long out_fs = (long)mm->cin(l) * (H_ >> l) * (W_ >> l);
        // the tail of a forward = the last decoder's convolution: PART_MAIN stops in front of it, PART_TAIL runs nothing else
        const bool lastj = j == L_ - 1;
        const int jpart = part == PART_ALL ? PART_ALL : (lastj ? part : (part == PART_MAIN ? PART_ALL : -1));
        if (jpart >= 0) {
            ProfScope ps(mm, "decoder", st);
            const bool fuse = lastj && pred_fusable(mm);               // V5.py:195-197 in the last conv's epilogue
            const float* skip = w.merged[l] + (long)f0 * in_fs;
            if (mm->cfg.skip_concat) {                                 // decoder = Sequential(1x1 fusion, UpsampleConvLayer)
                if (jpart != PART_TAIL)
                    BDE_TRY(run_concat_fuse(mm, mm->dec_fuse[j], skip, x, nf, mm->cout(l), (long)(H_ >> (l + 1)) * (W_ >> (l + 1)), st));
                x = w.fuse;
                skip = nullptr;
            }
            BDE_TRY(run_decoder(mm, j, x, skip, w.dec[j] + (long)f0 * out_fs, nf,
                                H_ >> (l + 1), W_ >> (l + 1), st,
                                fuse ? w.head + (long)f0 * mm->cfg.basechannels * H_ * W_ : nullptr,
                                fuse ? w.out + (long)f0 * H_ * W_ : nullptr, jpart, T_ * B_));
        }
        x = w.dec[j] + (long)f0 * out_fs;
    }
    if (part == PART_MAIN) return BDE_OK;
    if (pred_fusable(mm)) return BDE_OK;
    const long total = (long)nf * H_ * W_;
    long blocks = std::min<long>(cdivl(total, 256), 4096);
    ProfScope ps(mm, "pred", st);
    const float* hd = w.head + (long)f0 * mm->cfg.basechannels * H_ * W_;
    if (mm->cfg.skip_concat) {                                     // predI = Sequential(1x1 fusion of cat(x, head), 1x1)
        BDE_TRY(run_concat_fuse(mm, mm->pred_fuse, x, hd, nf, mm->cfg.basechannels, (long)H_ * W_, st));
        x = w.fuse;
        hd = nullptr;
    }
    hipLaunchKernelGGL(pred_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x,
                       hd, mm->P(mm->predw_off),
                       mm->P(mm->predb_off), w.out + (long)f0 * H_ * W_, mm->cfg.basechannels, (long)H_ * W_, total,
                       mm->cfg.activation);
    BDE_HIP(hipGetLastError());
    return BDE_OK;
}

static bool side_decode_on(const bde_model* m, int T) {
    const bde_config& c = m->cfg;
    const bool plain_flags = c.use_rc && c.recurrent_type == 0 && !c.skip_concat && c.depths[c.num_encoders - 1] > 0;
    return m->overlap != 0 && plain_flags && !(m->debug_skip & (2 | 8)) && !m->prof_on && T > m->overlap_chunk;
}

static int forward_body(bde_model* m, int T, int B, int H, int W, hipStream_t s, int part) {
    const bde_config& c = m->cfg;
    Workspace& ws = m->W();
    const int L = c.num_encoders;
    const long TB = (long)T * B;
    // While the attention chain of the LAST level walks the frames one by one (V5.py:154-169), the decoder of the frames already
    // refined -- independent per frame, V5.py:183-202 -- runs on a side stream in chunks of `overlap_chunk` frames: a forked branch
    // of the captured graph.  The chain's launches are latency-bound and leave most of the chip idle; the decoder's are not.  The
    // last chunk stays on the main stream (it is what the forward's tail is cut from).  Results are bit-identical: same launches.
    const bool side_decode = side_decode_on(m, T);
    const int last_chunk_t0 = side_decode ? (T - 1) / m->overlap_chunk * m->overlap_chunk : 0;
    const int tail_f0 = last_chunk_t0 * B, tail_nf = (int)TB - tail_f0;
    if (part == PART_TAIL) return (m->debug_skip & 8) ? BDE_OK : decode_frames(m, tail_f0, tail_nf, T, B, H, W, s, PART_TAIL);
    // A. head (V5.py:116) and the first level's encoder convolution: PART_PRE
    if (part != PART_MAIN) {
        { ProfScope ps(m, "head", s); BDE_TRY(run_head_conv(m, ws.ev, ws.head, (int)TB, H, W, s)); }
        if (!(m->debug_skip & 16)) BDE_TRY(run_enc_gx(m, 0, ws.head, 0, (int)TB, T, B, H, W, s));
        if (part == PART_PRE) return BDE_OK;
    }
    // B. levels (V5.py:119-172)
    struct SideCtx { int T, B, H, W, chunk, slot; hipStream_t main, side; };
    static auto decode_fn = decode_frames;     // (plain function pointer for the captureless callback)
    const int slot = (m->cap_stream && s == m->cap_stream) ? bde_model::MAX_SLOTS : m->cur;   // (capturing: the capture-only set)
    if (side_decode && !m->side[slot]) {
        int lo = 0, hi = 0;                               // lowest priority: the chain on the main stream goes first
        BDE_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        BDE_HIP(hipStreamCreateWithPriority(&m->side[slot], hipStreamNonBlocking, lo));
        BDE_HIP(hipEventCreateWithFlags(&m->join_ev[slot], hipEventDisableTiming));
    }
    while (side_decode && (int)m->frame_ev[slot].size() < T) {
        hipEvent_t e;
        BDE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m->frame_ev[slot].push_back(e);
    }
    const float* target = ws.head;
    bool decoded = false;
    for (int l = 0; l < L; ++l) {
        const int Hl = H >> l, Wl = W >> l, h = Hl / 2, w = Wl / 2, C = m->cout(l);
        BDE_TRY(run_recurrent_level(m, l, target, T, B, Hl, Wl, s, /*enc_done=*/l == 0));
        const long n = TB * C * h * w;
        { ProfScope ps(m, pname("merge", l), s); BDE_TRY(add2(ws.hseq[l], ws.hseq[l] + n, ws.merged[l], n, s)); }   // V5.py:137-147
        if (c.depths[l] > 0 && !(m->debug_skip & (l == 0 ? 1 : 2))) {
            static const char* names[BDE_MAX_LEVELS] = {"attn0", "attn1", "attn2", "attn3", "attn4", "attn5", "attn6", "attn7"};
            ProfScope ps(m, names[l], s);
            SideCtx sc{T, B, H, W, m->overlap_chunk, slot, s, m->side[slot]};
            FrameDoneFn fn = nullptr;
            const bool fork = side_decode && l == L - 1;
            if (fork) {
                fn = [](bde_model* mm, int t, void* vp) -> int {
                    SideCtx* q = (SideCtx*)vp;
                    const int done = t + 1;
                    if (done % q->chunk != 0 || done > (q->T - 1) / q->chunk * q->chunk) return BDE_OK;   // (the last chunk: main stream)
                    const int t0 = done - q->chunk;
                    BDE_HIP(hipEventRecord(mm->frame_ev[q->slot][t], q->main));
                    BDE_HIP(hipStreamWaitEvent(q->side, mm->frame_ev[q->slot][t], 0));
                    return decode_fn(mm, t0 * q->B, q->chunk * q->B, q->T, q->B, q->H, q->W, q->side, PART_ALL);
                };
            }
            BDE_TRY(run_attention_level(m, l, T, B, h, w, s, fn, &sc));
            if (fork) {
                BDE_HIP(hipEventRecord(m->join_ev[slot], m->side[slot]));
                BDE_HIP(hipStreamWaitEvent(s, m->join_ev[slot], 0));
                decoded = true;
            }
        }
        if (l == L - 1 && c.depths[l] == 0) BDE_TRY(run_bottleneck_level(m, l, T, B, h, w, s));
        target = ws.merged[l];
    }
    if (m->debug_skip & 8) return BDE_OK;
    // C. decoder: every frame, or the last chunk behind a forked decode; PART_MAIN stops in front of its last convolution
    const int dpart = part == PART_MAIN ? PART_MAIN : PART_ALL;
    if (decoded) return decode_frames(m, tail_f0, tail_nf, T, B, H, W, s, dpart);
    return decode_frames(m, 0, (int)TB, T, B, H, W, s, dpart);
}

static int validate_config(const bde_config* c) {
    BDE_REQUIRE(c != nullptr, "null config");
    BDE_REQUIRE(c->num_encoders >= 1 && c->num_encoders <= BDE_MAX_LEVELS, "num_encoders=%d", c->num_encoders);
    BDE_REQUIRE(c->num_bins >= 1 && c->basechannels >= 1, "num_bins=%d basechannels=%d", c->num_bins, c->basechannels);
    BDE_REQUIRE(c->ks == 3 || c->ks == 5, "ks=%d (3 or 5)", c->ks);
    BDE_REQUIRE(c->frame_num >= 1 && c->frame_num <= BDE_MAX_FRAMES, "frame_num=%d", c->frame_num);
    BDE_REQUIRE(c->q_idx >= 0 && c->q_idx < c->frame_num, "q_idx=%d", c->q_idx);
    BDE_REQUIRE(c->buffer_index[c->q_idx] == 0, "buffer_index[q_idx] must be 0 (the query frame is the current frame)");
    BDE_REQUIRE(c->activation == 0 || c->activation == 1, "activation=%d", c->activation);
    BDE_REQUIRE(c->recurrent_type == 0 || c->recurrent_type == 1, "recurrent_type=%d (0 ConvLSTM, 1 ConvGRU)", c->recurrent_type);
    BDE_REQUIRE(c->use_rc == 0 || c->use_rc == 1, "use_rc=%d", c->use_rc);
    BDE_REQUIRE(c->skip_concat == 0 || c->skip_concat == 1, "skip_concat=%d", c->skip_concat);
    BDE_REQUIRE(c->norm >= 0 && c->norm <= 2, "norm=%d (0 none, 1 BN, 2 IN)", c->norm);
    BDE_REQUIRE(c->num_res_blocks >= 0 && c->num_res_blocks <= 64, "num_res_blocks=%d", c->num_res_blocks);
    for (int l = 0; l < c->num_encoders; ++l) {
        BDE_REQUIRE(c->depths[l] >= 0, "depths[%d]=%d", l, c->depths[l]);
        if (c->depths[l] > 0) {
            const int C = c->basechannels << (l + 1);
            BDE_REQUIRE(c->num_heads >= 1 && C % c->num_heads == 0, "C=%d not divisible by %d heads", C, c->num_heads);
            const int hd = C / c->num_heads;
            BDE_REQUIRE(hd == 1 || hd == 2 || hd == 4 || hd == 8 || hd == 16 || hd == 32, "head_dim=%d not built", hd);
        }
    }
    return BDE_OK;
}


}  // namespace bde
