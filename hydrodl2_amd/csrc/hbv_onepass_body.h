// hbv_onepass_body.h -- the statements of the one-pass static adjoint's kernels, included INSIDE the braces of
// k_bwd_chunk_onepass (all four rows of grad_flux4: LIVE = 4) and of k_bwd_chunk_onepass_live (the leading LIVE < 4
// rows, runoff-only loss) in hbv_chunked.h, which define BETAET, GFULL and LIVE as constant expressions and name the
// kernel argument A.  One text for both, and no function in between: the adjoint's arithmetic is compiled with
// contraction allowed (HBVX_ADJ_FMA, hbv_step.h), so which product of a sum the compiler fuses depends on the shape
// of the code around it -- moving these statements into an inlined function changed the rounding of the four-row
// kernel's gradient (tests/test_chunk_fold_bits_gpu.py pins its bits).  Not a header to include anywhere else.
    static_assert(LIVE >= 1 && LIVE <= 4 && (LIVE == 4 || !GFULL), "fewer live rows: the runoff-only loss");
    extern __shared__ float onepass_slot[];
    constexpr int MODEL = MODEL_HBV10, DYN = 0;
    constexpr int NP = ChunkNP<MODEL, BETAET>::value;
    typedef Step<MODEL, BETAET> S;
    const int ds_[3] = {0, 0, 0};
    const hbvx_desc &d = A.d;
    const hbvx_bwd_io &io = A.io;
    ChunkBlock blk;
    if (!chunk_block(d, A.lgMp, A.per_xcd, blk)) return;
    const LaneId L = lane_id(d, A.lgMp, blk.bx);
    const int grp = blk.chunk;                                              // the block map deals groups
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);    // wave of the workgroup
    const int nw = min(min(A.group, ONEPASS_GMAX), A.nchunk - grp * A.group);   // waves of this group with a chunk
    const int chunk = grp * A.group + w;
    const int t0 = chunk * A.C, t1 = min(d.T, t0 + A.C);
    const int64_t N = (int64_t)d.B * d.M;
    const bool raw = d.raw_sigmoid != 0;
    const float nz = d.nearzero, invM = 1.0f / (float)d.M;
    float usta[NP], psta[NP];
    bool use_dyn[NP];
    chunk_static<NP, DYN>(d, L, raw, usta, psta, use_dyn, 0, ds_);

    float Phi[5][5], phi[5];
    float G[6][NPARAM_MAX];   // G[k]: Jθ^T sums of the unit vector Phi[k]; G[5]: of the offset (entries never touched fold away)
#pragma unroll
    for (int k = 0; k < 5; k++) {
        phi[k] = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; i++) Phi[k][i] = (i == k) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
        for (int i = 0; i < NPARAM_MAX; i++) G[k][i] = 0.0f;
    if (w < nw) {   // (a wave past the record's last chunk has no days: nothing to load)
    ChunkRaw<NP> Rn;
    chunk_issue<NP, DYN, GFULL, false, false, LIVE>(d, io, L, t1 - 1, io.n_flux, Rn, 0, ds_);
    for (int t = t1 - 1; t >= t0; t--) {
        ChunkRaw<NP> Rc = Rn;
        if (t > t0) chunk_issue<NP, DYN, GFULL, false, false, LIVE>(d, io, L, t - 1, io.n_flux, Rn, 0, ds_);   // next day's loads in flight
        ChunkDay<MODEL, BETAET, NP> D;
        chunk_finish<MODEL, BETAET, NP, DYN, GFULL>(d, Rc, raw, nz, 0.0f, 0.0f, usta, psta, use_dyn, io.n_flux, invM,
                                                    D, 0, ds_, LIVE < 4 || io.grad_flux4 != nullptr);
        const typename S::JT c = D.s.jt_coef(D.p, nz);
        const typename S::JG k = D.s.jg_coef(D.p, nz);
        S::template jt_gp<0>(c, k, Phi[0], G[0]);
        S::template jt_gp<0>(c, k, Phi[1], G[1]);
        S::template jt_gp<1>(c, k, Phi[2], G[2]);
        S::template jt_gp<2>(c, k, Phi[3], G[3]);
        S::template jt_gp<2>(c, k, Phi[4], G[4]);
        if constexpr (!GFULL) {
            S::template jt_gp<2, true>(c, k, phi, G[5], D.g.gQ0 + D.g.gQ, D.g.gQ1 + D.g.gQ, D.g.gQ2 + D.g.gQ);
        } else {
            float gx[3];
            D.s.bwd(D.p, nz, D.g, phi, G[5], gx);   // its gp output is g0_c
        }
    }
    }
    OnepassRows<NP> rows{A.phi + ((int64_t)grp * 30) * N + L.n, A.gpart + ((int64_t)grp * onepass_rows(NP)) * N + L.n, N,
                         L.active};
    if (A.group == 1) {
        onepass_put<float, NP>(Phi, phi, G, rows);
        return;
    }
    // Hand-over, latest chunk first: the last wave with a chunk puts its map into the slot, then stage s belongs to wave
    // s.  nw and s are the same for every wave of the workgroup, so all of them (those without a chunk too) meet at
    // every barrier.
    OnepassSlot<NP> slot{onepass_slot + (threadIdx.x & 63)};
    if (w == nw - 1 && w > 0) onepass_put<float, NP>(Phi, phi, G, slot);
    // (Written out stage by stage and nested, so that no stage tests nw again behind a barrier: as a loop over s, or as
    // three tests in a row, the compiler lays branches back across the compositions and the day loop is no longer the
    // kernel's largest loop.)
    static_assert(ONEPASS_GMAX == 4, "one stage per wave above wave 0");
    if (nw > 1) {
        if (nw > 2) {
            if (nw > 3) __syncthreads();                                      // stage 3: wave 3 has put its map
            if (w == 2 && nw > 3) onepass_compose<float, NP, false>(slot, Phi, phi, G, slot);
            __syncthreads();
        }
        if (w == 1 && nw > 2) onepass_compose<float, NP, false>(slot, Phi, phi, G, slot);
        __syncthreads();
    }
    if (w == 0) {
        if (nw == 1) onepass_put<float, NP>(Phi, phi, G, rows);
        else onepass_compose<float, NP, true>(slot, Phi, phi, G, rows);
    }
