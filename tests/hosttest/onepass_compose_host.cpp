// onepass_compose_host.cpp -- TEST HARNESS: the composition of the one-pass static adjoint's chunk maps
// (hydrodl2_amd/csrc/hbv_onepass_compose.h, hbvx::onepass_compose) on the host, in its double instantiation, so
// tests/test_onepass_compose_host.py can check it without a GPU: a chain of chunk maps applied hop by hop against the
// same chain composed into one map and applied once.  Built only by that test; never shipped or loaded by the package.
#include "../../hydrodl2_amd/csrc/hbv_onepass_compose.h"

using namespace hbvx;

namespace {

struct Map {                       // one chunk's rows, dense (entries outside the sparsity patterns are zero)
    double Phi[5][5], phi[5], G[6][NPARAM_MAX];
};
struct Src {
    const Map *m;
    double Phi(int k, int j) const { return m->Phi[k][j]; }
    double phi(int j) const { return m->phi[j]; }
    double G(int k, int p) const { return m->G[k][p]; }
};
struct Dst {
    Map *m;
    void Phi(int k, int i, double v) { m->Phi[k][i] = v; }
    void phi(int i, double v) { m->phi[i] = v; }
    void G(int k, int p, double v) { m->G[k][p] = v; }
};

void load(Map &m, const double *Phi, const double *phi, const double *G)
{
    for (int k = 0; k < 5; k++) {
        m.phi[k] = phi[k];
        for (int i = 0; i < 5; i++) m.Phi[k][i] = Phi[k * 5 + i];
    }
    for (int k = 0; k < 6; k++)
        for (int p = 0; p < NPARAM_MAX; p++) m.G[k][p] = G[k * NPARAM_MAX + p];
}

// a_out = phi + a Phi, g += G a + g0 -- dense sums, no knowledge of the patterns
template <int NP>
void apply(const Map &m, double *a, double *g)
{
    double an[5];
    for (int p = 0; p < NP; p++) {
        double v = m.G[5][p];
        for (int k = 0; k < 5; k++) v += m.G[k][p] * a[k];
        g[p] += v;
    }
    for (int i = 0; i < 5; i++) {
        double v = m.phi[i];
        for (int k = 0; k < 5; k++) v += a[k] * m.Phi[k][i];
        an[i] = v;
    }
    for (int i = 0; i < 5; i++) a[i] = an[i];
}

template <int NP>
void chain(int n, const double *Phi, const double *phi, const double *G, const double *a_in, double *g_hop,
           double *a_hop, double *g_one, double *a_one, double *cPhi, double *cphi, double *cG)
{
    for (int p = 0; p < NPARAM_MAX; p++) g_hop[p] = g_one[p] = 0.0;
    // route A: hop chunk by chunk, last chunk first
    for (int i = 0; i < 5; i++) a_hop[i] = a_in[i];
    for (int c = n - 1; c >= 0; c--) {
        Map m;
        load(m, Phi + c * 25, phi + c * 5, G + c * 6 * NPARAM_MAX);
        apply<NP>(m, a_hop, g_hop);
    }
    // route B: fold the chain into one map, last chunk first, and apply it once (onepass_compose writes the rows inside
    // the patterns and Phi's zeros; the rest of G is never a row of the workspace and starts as zero here)
    Map comp;
    load(comp, Phi + (n - 1) * 25, phi + (n - 1) * 5, G + (n - 1) * 6 * NPARAM_MAX);
    for (int c = n - 2; c >= 0; c--) {
        Map e, r;
        load(e, Phi + c * 25, phi + c * 5, G + c * 6 * NPARAM_MAX);
        for (int k = 0; k < 6; k++)
            for (int p = 0; p < NPARAM_MAX; p++) r.G[k][p] = 0.0;
        Src s{&comp};
        Dst d{&r};
        onepass_compose<double, NP, true>(s, e.Phi, e.phi, e.G, d);
        comp = r;
    }
    for (int i = 0; i < 5; i++) a_one[i] = a_in[i];
    apply<NP>(comp, a_one, g_one);
    for (int k = 0; k < 5; k++) {
        cphi[k] = comp.phi[k];
        for (int i = 0; i < 5; i++) cPhi[k * 5 + i] = comp.Phi[k][i];
    }
    for (int k = 0; k < 6; k++)
        for (int p = 0; p < NPARAM_MAX; p++) cG[k * NPARAM_MAX + p] = comp.G[k][p];
}

} // namespace

// Phi [n][5][5], phi [n][5], G [n][6][NPARAM_MAX] (row 5: g0), a_in [5]; out: the gradient [NPARAM_MAX] and the leaving
// adjoint [5] of both routes, and the composite's rows.  Returns NPARAM_MAX.
extern "C" int onepass_chain(int np, int n, const double *Phi, const double *phi, const double *G, const double *a_in,
                             double *g_hop, double *a_hop, double *g_one, double *a_one, double *cPhi, double *cphi,
                             double *cG)
{
    if (np == 12) chain<12>(n, Phi, phi, G, a_in, g_hop, a_hop, g_one, a_one, cPhi, cphi, cG);
    else if (np == 13) chain<13>(n, Phi, phi, G, a_in, g_hop, a_hop, g_one, a_one, cPhi, cphi, cG);
    else return -1;
    return NPARAM_MAX;
}

// the patterns, for the test's draws: G[k][p] may be non-zero for k >= kmin(p), Phi[k][i] for i < reach(k)
extern "C" int onepass_pattern_kmin(int p) { return onepass_kmin(p); }
extern "C" int onepass_pattern_reach(int k) { return onepass_reach(k); }
