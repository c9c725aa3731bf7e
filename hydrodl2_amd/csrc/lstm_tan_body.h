// lstm_tan_body.h -- the body of the tangent-linear LSTM kernels k_lstm_tan and k_lstm_dirs (lstm_seq.h), included
// into both after their prologue: template parameters H and UG, KQ = H / 64, the LDS array `part`, the LstmTanArgs `a`
// (pointing at the direction's tangent buffers and slabs), the row tile `tile` and the workgroup's index `s` in it.
// One text, so that a (direction, row tile) pair of k_lstm_dirs runs what k_lstm_tan runs for that direction,
// operation for operation, and k_lstm_tan's code is what it was before the second kernel existed.
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, kq = l >> 4, n = l & 15;
    const bool fin = w < UG;
    const int wg = fin ? w : 0;                        // the unit group whose cell this wave computes
    const int u0 = (s * UG + wg) * 4;
    const int unit = u0 + kq;
    const int row = tile * LSTM_ROWS + n, rowc = row < a.B ? row : a.B - 1;
    const bool live = row < a.B && fin;

    float wreg[UG][KQ * 4];                            // A operands exactly as in k_lstm_fwd
    {
        const int m = l & 15;
#pragma unroll
        for (int g = 0; g < UG; ++g) {
            const float *wr = a.w_hh + (size_t)((m & 3) * H + (s * UG + g) * 4 + (m >> 2)) * H + 4 * (w * (H / 16) + kq);
#pragma unroll
            for (int j = 0; j < KQ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) wreg[g][j * 4 + i] = wr[16 * j + i];
        }
    }
    const size_t slab = (size_t)H * LSTM_ROWS;
    __shared__ int timed_out;                           // as in k_lstm_fwd: raised before the barrier, acted on after it
    if (threadIdx.x == 0) timed_out = 0;
    __syncthreads();
    const bool publish = (int)blockIdx.x != a.drop_wg;
    const size_t e0 = (size_t)rowc * H + unit;
    float cd = a.c0_t ? a.c0_t[e0] : 0.0f;             // c'_{t-1}
    float cp = a.c0 ? a.c0[e0] : 0.0f;                 // c_{t-1}
    // A step's inputs are loaded in the step before it, into the register set the step will read: the time loop
    // runs two steps per iteration on two sets.  (One set carried around the loop costs register copies, and a copy
    // of a loaded register waits for the load -- vmcnt counts in order, so for everything issued before it too, the
    // hand-off store included.)  The multiplying waves load and compute the cell of unit group 0 along with the
    // finishing waves and store nothing: with no branch around them, every path reads the set it loaded and the
    // compiler has no load left to wait for when it issues the next ones.
    struct In { lstm_f4 z, g; float c; };               // gx'_t, gates_t, c_t
    auto load = [&](int t, In &in) {
        const size_t e = (size_t)t * a.B * H + e0;
        in.z = *reinterpret_cast<const lstm_f4 *>(a.gx_t + e * 4);
        in.g = *reinterpret_cast<const lstm_f4 *>(a.gates + e * 4);
        in.c = a.c_all[e];
    };
    // one step; false: the hand-off timed out (outputs poisoned), the workgroup leaves
    auto step = [&](int t, const In &cur, In &nxt) -> bool {
        const bool mul = t > 0 || a.h0_t;             // h'_{t-1} W_hh^T is not zero
        lstm_f4 hv[KQ];
        if (mul) {
            // step 0 with a tangent on h0 takes it through the same MFMA chain and LDS sum, as k_lstm_fwd takes h0
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < KQ; ++j)
                    hv[j] = *reinterpret_cast<const lstm_f4 *>(a.h0_t + (size_t)rowc * H + 4 * (w * (H / 16) + 4 * j + kq));
            } else if (!lstm_fetch<KQ>(a, a.xch + ((size_t)(t - 1) * a.ntile + tile) * slab, (int)(slab * 4), w * (H / 16), kq, n, hv))
                timed_out = 1;
        }
        // This step's set and h'_{t-1} are complete here on every path (behind a hand-off, its own wait has covered
        // them), so nothing below waits on a load; the next step's set is issued behind this hand-off and waited for
        // by the next one, a step later.
        asm volatile("" ::"v"(cur.z), "v"(cur.g), "v"(cur.c));
        if (mul) {
#pragma unroll
            for (int j = 0; j < KQ; ++j) asm volatile("" ::"v"(hv[j]));
        }
        if (t + 1 < a.T) load(t + 1, nxt);
        lstm_f4 acc = {0, 0, 0, 0};
        if (mul) {
            lstm_f4 p[UG];
#pragma unroll
            for (int g = 0; g < UG; ++g) p[g] = lstm_f4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < KQ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int g = 0; g < UG; ++g)
                        p[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[g][j * 4 + i], hv[j][i], p[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < UG; ++g) part[t & 1][w][g][l] = p[g];
            __syncthreads();                            // the only barrier of a step; part[] is two deep
            if (timed_out) {
                if (live) {
                    a.h_t[((size_t)(a.T - 1) * a.B + row) * H + unit] = __builtin_nanf("");
                    if (a.c_t_last) a.c_t_last[e0] = __builtin_nanf("");
                }
                return false;
            }
            acc = (part[t & 1][0][wg][l] + part[t & 1][1][wg][l]) + (part[t & 1][2][wg][l] + part[t & 1][3][wg][l]);
        }
        acc += cur.z;
        const float ig = cur.g[0], fg = cur.g[1], gg = cur.g[2], og = cur.g[3];
        const float di = ig * (1.0f - ig) * acc[0], df = fg * (1.0f - fg) * acc[1];
        const float dg = (1.0f - gg * gg) * acc[2], dout = og * (1.0f - og) * acc[3];
        cd = df * cp + fg * cd + di * gg + ig * dg;
        cp = cur.c;
        const float tau = lstm_tanh(cur.c);
        const float hd = dout * tau + og * (1.0f - tau * tau) * cd;
        if (live) {
            a.h_t[(size_t)t * a.B * H + e0] = hd;
            if (t == a.T - 1 && a.c_t_last) a.c_t_last[e0] = cd;
        }
        if (fin && t + 1 < a.T && publish) {
            float *xp = a.xch + ((size_t)t * a.ntile + tile) * slab + ((size_t)(u0 >> 2) * LSTM_ROWS + n) * 4 + kq;
            __hip_atomic_store(xp, hd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return true;
    };
    In in0 = {{0, 0, 0, 0}, {0, 0, 0, 0}, 0.0f}, in1 = in0;
    load(0, in0);
    // (the loop is left right after the step that has no successor: a path that skipped a step to reach the loop
    // head would carry that step's set, unread, into the next load of it)
    for (int t = 0;; t += 2) {
        if (!step(t, in0, in1) || t + 1 == a.T) return;
        if (!step(t + 1, in1, in0) || t + 2 == a.T) return;
    }
