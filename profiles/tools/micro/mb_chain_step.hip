// What does a step of the stitch's chain cost in each form of handing the rescaled vector round (kernels_stitch.hpp,
// ChainForm)?  The library's own k_chain<NP, D, FORM> on the stitch's shape: one wavefront per workgroup, ~400 chains
// (RUNS runs x N basis vectors, the chains of a run share its operators, which stay in L2), 12 steps.  A step is priced
// as (12-step launch - 2-step launch) / 10, from the minima of the rounds; every form's output is compared bit for bit with the LDS form's.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o mb profiles/tools/micro/mb_chain_step.hip && ./mb
#include "../../../imcoalhmm_amd/csrc/kernels_stitch.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static const char *kForms[] = {"LDS write + broadcast reads", "v_readlane pair", "lane swaps + v_mov_b64_dpp"};
constexpr int STEPS = 12, SHORT = 2, LAUNCHES = 200, ROUNDS = 7;

template <int NP, int D, int FORM>
int run_form(int N, int runs, int steps, const double *dP, const int *dEX, double *dPo, int *dEXo, ChainDesc *dC,
             std::vector<double> &Po, std::vector<int> &EXo, double us[3])
{
    const int chains = runs * N;
    std::vector<ChainDesc> cd((size_t)chains);
    for (int r = 0; r < runs; ++r)
        for (int c = 0; c < N; ++c)   // an operator run of `steps` units; unit t of run r is vectors (r*STEPS + t)*N ...
            cd[(size_t)r * N + c] = ChainDesc{(uint32_t)(r * STEPS), (uint32_t)(r * STEPS + steps), (uint32_t)c, (uint32_t)(r * N + c), 0u, 0u, 0u, (uint32_t)(r * STEPS * N)};
    CHECK(hipMemcpy(dC, cd.data(), cd.size() * sizeof(ChainDesc), hipMemcpyHostToDevice));
    const uint32_t n_vecs = (uint32_t)(runs * STEPS * N);
    auto launch = [&]() {
        hipLaunchKernelGGL((k_chain<NP, D, FORM>), dim3(chains), dim3(64), 0, 0, dC, N, (uint32_t)(runs * STEPS), n_vecs, dP, dEX, dEX,
                           (uint32_t)chains, dPo, dEXo, (double *)nullptr, 0);
    };
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int k = 0; k < 20; ++k) launch();
    std::vector<double> t;
    for (int r = 0; r < ROUNDS; ++r) {
        CHECK(hipEventRecord(e0));
        for (int k = 0; k < LAUNCHES; ++k) launch();
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        t.push_back(ms * 1e3 / LAUNCHES);
    }
    std::sort(t.begin(), t.end());
    us[0] = t.front(); us[1] = t[t.size() / 2]; us[2] = t.back();
    Po.resize((size_t)chains * NP); EXo.resize((size_t)chains);
    CHECK(hipMemcpy(Po.data(), dPo, Po.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(EXo.data(), dEXo, EXo.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return 0;
}

template <int NP, int D>
int run_shape(int N)
{
    const int runs = (400 + N - 1) / N, chains = runs * N;
    const size_t n_vecs = (size_t)runs * STEPS * N;
    std::mt19937_64 rng(12345 + NP);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> P(n_vecs * NP, 0.0);
    std::vector<int> EX(n_vecs);
    for (size_t v = 0; v < n_vecs; ++v) {
        for (int c = 0; c < N; ++c) P[v * NP + c] = u(rng) / N;
        EX[v] = -(int)(rng() % 40);
    }
    double *dP, *dPo; int *dEX, *dEXo; ChainDesc *dC;
    CHECK(hipMalloc(&dP, P.size() * 8)); CHECK(hipMalloc(&dEX, EX.size() * 4));
    CHECK(hipMalloc(&dPo, (size_t)chains * NP * 8)); CHECK(hipMalloc(&dEXo, (size_t)chains * 4)); CHECK(hipMalloc(&dC, (size_t)chains * sizeof(ChainDesc)));
    CHECK(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dEX, EX.data(), EX.size() * 4, hipMemcpyHostToDevice));
    printf("NP = %d (N = %d, D = %d): %d chains of %d steps, operators %.0f KB\n", NP, N, D, chains, STEPS, n_vecs * NP * 8 / 1024.0);
    std::vector<double> ref, got; std::vector<int> refe, gote;
    int rc = 0;
    auto form = [&](auto F) {
        constexpr int FORM = decltype(F)::value;
        double lng[3], sht[3];
        CHECK(hipMemset(dPo, 0, (size_t)chains * NP * 8));
        if (run_form<NP, D, FORM>(N, runs, SHORT, dP, dEX, dPo, dEXo, dC, got, gote, sht)) return 1;
        CHECK(hipMemset(dPo, 0, (size_t)chains * NP * 8));
        if (run_form<NP, D, FORM>(N, runs, STEPS, dP, dEX, dPo, dEXo, dC, got, gote, lng)) return 1;
        if (FORM == CHAIN_LDS) { ref = got; refe = gote; }
        const bool same = std::memcmp(ref.data(), got.data(), ref.size() * 8) == 0 && std::memcmp(refe.data(), gote.data(), refe.size() * 4) == 0;
        printf("  %-30s launch of %2d steps %6.2f / %6.2f / %6.2f us (min / median / max of %d x %d), of %d steps %6.2f / %6.2f / %6.2f | step %.3f us | %s\n",
               kForms[FORM], STEPS, lng[0], lng[1], lng[2], ROUNDS, LAUNCHES, SHORT, sht[0], sht[1], sht[2], (lng[0] - sht[0]) / (STEPS - SHORT),
               same ? "bits equal to the LDS form" : "DIFFERS from the LDS form");
        if (!same) rc = 2;
        return 0;
    };
    if (form(std::integral_constant<int, CHAIN_LDS>()) || form(std::integral_constant<int, CHAIN_LANE>()) || form(std::integral_constant<int, CHAIN_DPP>()))
        return 1;
    CHECK(hipFree(dP)); CHECK(hipFree(dEX)); CHECK(hipFree(dPo)); CHECK(hipFree(dEXo)); CHECK(hipFree(dC));
    return rc;
}

int main()
{
    int rc = run_shape<20, 4>(20);
    if (rc == 1) return 1;
    const int rc2 = run_shape<64, 2>(64);
    return rc2 ? rc2 : rc;
}
