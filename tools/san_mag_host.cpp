// Host sanitizer check of the magnitude family's host forms and trpl_interp_rows (no device needed): the four host-loop exports on
// tiny arrays (S = 5, C = 2, M = 3), the n_obs forms against the _w forms given wsum = (double)n_obs bit for bit, and the refusals
// of all eight exports, which return before anything is launched.  Build the two units it exercises with the sanitizers and link
// the library's other objects as they are (from bayesian-inference-trpl_amd, after `make`):
//   F="-O1 -g -fPIC -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c csrc/trpl_api.hip -o /tmp/api.o && hipcc $F -ffp-contract=off -c csrc/likelihood.hip -o /tmp/lik.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c ../tools/san_mag_host.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 /tmp/main.o /tmp/api.o /tmp/lik.o $(ls csrc/build/*.o | grep -v -e trpl_api.o -e likelihood.o) \
//       -fsanitize=address,undefined -ldl -o /tmp/san_mag_host && /tmp/san_mag_host
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/trpl.h"

static int failures = 0;
#define EXPECT(cond)                                                                     \
    do {                                                                                 \
        if (!(cond)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, trpl_last_error()); failures++; } \
    } while (0)

int main()
{
    const int64_t S = 5, M = 3;
    const int32_t C = 2;
    // exactly-sized heap arrays: one element past any of them is a sanitizer report
    std::vector<double> sse(C * S), esum(C * S), off = {-0.25, 0.0, 0.5}, wsum = {7.0, 3.0};
    std::vector<int64_t> n_obs = {7, 3};
    for (int i = 0; i < C * S; i++) { sse[i] = 1.0 + 0.37 * i; esum[i] = 0.11 * i - 0.4; }
    sse[3] = INFINITY;                                   // a flagged system

    std::vector<double> Pn(M * S, -1.0), Pw(M * S, -1.0);
    EXPECT(trpl_mag_grid(sse.data(), esum.data(), n_obs.data(), S, C, off.data(), M, Pn.data()) == TRPL_OK);
    EXPECT(trpl_mag_grid_w(sse.data(), esum.data(), wsum.data(), S, C, off.data(), M, Pw.data()) == TRPL_OK);
    EXPECT(memcmp(Pn.data(), Pw.data(), Pn.size() * 8) == 0);
    for (uint32_t flags : {0u, (uint32_t)TRPL_MAG_PER_CURVE}) {
        const size_t nb = flags ? C * S : S;
        std::vector<double> bn(nb, 9.0), bw(nb, 9.0), pn(S, -1.0), pw(S, -1.0);
        EXPECT(trpl_mag_profile(sse.data(), esum.data(), n_obs.data(), S, C, flags, bn.data(), pn.data()) == TRPL_OK);
        EXPECT(trpl_mag_profile_w(sse.data(), esum.data(), wsum.data(), S, C, flags, bw.data(), pw.data()) == TRPL_OK);
        EXPECT(memcmp(bn.data(), bw.data(), nb * 8) == 0 && memcmp(pn.data(), pw.data(), S * 8) == 0);
    }

    // refusals: each returns before a host loop or a launch
    std::vector<double> P(M * S, 0.0), best(C * S, 0.0), bad_w = {1.0, -1.0}, nan_w = {NAN, 1.0};
    std::vector<int64_t> bad_n = {7, 0};
    const double *s = sse.data(), *e = esum.data(), *o = off.data();
    EXPECT(trpl_mag_grid(s, e, n_obs.data(), S, C, o, -1, P.data()) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid(s, e, nullptr, S, C, o, M, P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "n_obs must not be NULL"));
    EXPECT(trpl_mag_grid(s, e, bad_n.data(), S, C, o, M, P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "n_obs[1]=0"));
    EXPECT(trpl_mag_grid(s, e, n_obs.data(), S, C, nullptr, M, P.data()) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid_dev(s, e, n_obs.data(), S, 0, o, M, P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid_dev(s, e, bad_n.data(), S, C, o, M, P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid_dev(nullptr, e, n_obs.data(), S, C, o, M, P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid_w(s, e, bad_w.data(), S, C, o, M, P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "wsum[1]=-1"));
    EXPECT(trpl_mag_grid_w(s, e, nullptr, S, C, o, M, P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "wsum must not be NULL"));
    EXPECT(trpl_mag_grid_w_dev(s, e, nan_w.data(), S, C, o, M, P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_grid_w_dev(s, e, wsum.data(), S, TRPL_MAG_MAX_CURVES + 1, o, M, P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile(s, e, n_obs.data(), S, C, 2u, best.data(), P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "trpl_mag_profile: unknown"));
    EXPECT(trpl_mag_profile(s, e, n_obs.data(), S, C, 0u, nullptr, P.data()) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile_dev(s, e, n_obs.data(), S, C, 2u, best.data(), P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile_dev(s, e, n_obs.data(), S, C, 0u, best.data(), nullptr, nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile_w(s, e, wsum.data(), S, C, 2u, best.data(), P.data()) == TRPL_ERR_ARG && strstr(trpl_last_error(), "trpl_mag_profile_w: unknown"));
    EXPECT(trpl_mag_profile_w(s, e, bad_w.data(), S, C, 0u, best.data(), P.data()) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile_w_dev(s, e, wsum.data(), -1, C, 0u, best.data(), P.data(), nullptr) == TRPL_ERR_ARG);
    EXPECT(trpl_mag_profile_w_dev(s, e, wsum.data(), S, C, 0u, nullptr, P.data(), nullptr) == TRPL_ERR_ARG);
    for (double v : P) EXPECT(v == 0.0);                 // a refused call writes nothing

    // trpl_interp_rows: rows = 5, 4 columns (leading dimension 6), 3 observations, both element sizes
    const int64_t rows = 5, ncol = 4, ld = 6, n = 3;
    std::vector<double> pl8(rows * ld), dx = {0.25, 0.0, 1.0}, h = {1.0, 1.0, 1.0}, out8(rows * n), out4(rows * n);
    std::vector<float> pl4(rows * ld);
    std::vector<int32_t> hi = {1, 2, 3}, hi_bad = {1, 2, 4};
    for (int i = 0; i < rows * ld; i++) { pl8[i] = 0.5 * i; pl4[i] = (float)(0.5 * i); }
    EXPECT(trpl_interp_rows(pl8.data(), 8, rows, ncol, ld, hi.data(), dx.data(), h.data(), n, out8.data(), n) == TRPL_OK);
    EXPECT(trpl_interp_rows(pl4.data(), 4, rows, ncol, ld, hi.data(), dx.data(), h.data(), n, out4.data(), n) == TRPL_OK);
    EXPECT(memcmp(out8.data(), out4.data(), out8.size() * 8) == 0 && out8[0] == 0.125 && out8[(rows - 1) * n + 2] == 0.5 * ((rows - 1) * ld + 3));
    EXPECT(trpl_interp_rows(pl8.data(), 8, rows, ncol, ld, hi_bad.data(), dx.data(), h.data(), n, out8.data(), n) == TRPL_ERR_ARG);
    EXPECT(trpl_interp_rows(pl8.data(), 2, rows, ncol, ld, hi.data(), dx.data(), h.data(), n, out8.data(), n) == TRPL_ERR_ARG);
    EXPECT(trpl_interp_rows(pl8.data(), 8, rows, ncol, ld, hi.data(), dx.data(), h.data(), n, out8.data(), n - 1) == TRPL_ERR_ARG);
    EXPECT(trpl_interp_rows(nullptr, 8, rows, ncol, ld, hi.data(), dx.data(), h.data(), n, out8.data(), n) == TRPL_ERR_ARG);

    printf(failures ? "%d check(s) failed\n" : "san_mag_host: all checks passed\n", failures);
    return failures ? 1 : 0;
}
