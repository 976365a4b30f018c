// engine_sample.hpp - sampling from an HMM on the device: the checks both entry points share, and sample_on_device.
// Needs: engine_core.hpp; kernels_sample.hpp, sample_tiles.hpp, include/imcoal_sample.h; and PhaseTimer and allow_lds_budget,
// which imcoal_fwd.hip defines (chunk section, enqueue section) in front of the line that includes this header.
// Lock: sample_check makes no HIP call and needs no lock; check_device_output and sample_on_device expect g_mu held.
#pragma once

// ---- sampling from an HMM (include/imcoal_sample.h; csrc/sample_tiles.hpp is the specification) -------------------------
namespace {

uint64_t g_last_sampling[4] = {0, 0, 0, 0};   // imc_last_sampling: path, tiles, tile length, columns (g_mu held)

constexpr int SAMPLE_TILE_DEFAULT = 512;      // (profiles/device_sampling_ab.txt: the sweep over 64 .. 4096)

// every check both entry points share, before any HIP call; builds the threshold tables
int sample_check(const char *who, int N, int S, int emit, const double *pi, const double *T, const double *E, int R, size_t L,
                 const void *sym_out, int sym_bytes, imc::SampleTables *tb)
{
    const std::string w = std::string(who) + ": ";
    if (N < 1 || N > imc::kSampleMaxStates) return fail(IMC_ERR_ARG, w + "N must be in [1," + std::to_string(imc::kSampleMaxStates) + "]");
    if (S < 1 || S > imc::kSampleMaxSymbols) return fail(IMC_ERR_ARG, w + "S must be in [1," + std::to_string(imc::kSampleMaxSymbols) + "]");
    if (emit < 1 || emit > S) return fail(IMC_ERR_ARG, w + "emit_symbols must be in [1,S]");
    if (sym_bytes != 1 && sym_bytes != 2) return fail(IMC_ERR_ARG, w + "sym_bytes must be 1 or 2");
    if (sym_bytes == 1 && emit > 256) return fail(IMC_ERR_ARG, w + "byte symbols cannot carry more than 256 symbols");
    if (L < 1 || L >= (size_t)1 << 31) return fail(IMC_ERR_ARG, w + "L must be in [1,2^31)");
    if (R < 1 || R > imc::kSampleMaxReplicates) return fail(IMC_ERR_ARG, w + "n_replicates must be in [1," + std::to_string(imc::kSampleMaxReplicates) + "]");
    if (!pi || !T || !E) return fail(IMC_ERR_ARG, w + "pi, T or E is null");
    if (!sym_out) return fail(IMC_ERR_ARG, w + "the symbol output is null");
    if (sym_bytes == 2 && (reinterpret_cast<uintptr_t>(sym_out) & 1)) return fail(IMC_ERR_ARG, w + "16-bit symbol output is not 2-byte aligned");
    std::string err;
    if (!imc::build_tables(N, S, emit, pi, T, E, tb, &err)) return fail(IMC_ERR_ARG, w + err);
    return IMC_OK;
}

// `what` must be device memory of the library's device, `bytes` long: an error, never a fault (g_mu held, context ready)
int check_device_output(const void *p, size_t bytes, const char *what)
{
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(IMC_ERR_ARG, std::string(what) + " is not device memory (hipPointerGetAttributes)");
    }
    if (at.type != hipMemoryTypeDevice) return fail(IMC_ERR_ARG, std::string(what) + " is not device memory");
    if (at.device != g.device) return fail(IMC_ERR_ARG, std::string(what) + " is memory of device " + std::to_string(at.device) + ", the library runs on device " + std::to_string(g.device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess) {
        if ((const char *)p + bytes > (const char *)base + size) return fail(IMC_ERR_ARG, std::string(what) + ": the allocation ends before n_replicates x L elements");
    } else (void)hipGetLastError();
    return IMC_OK;
}

// The three launches on `st` (g_mu held, context ready, outputs checked); returns after synchronising st.
int sample_on_device(const imc::SampleTables &tb, uint64_t seed, uint32_t tag, uint64_t L, uint64_t total, uint32_t tile, uint32_t ntiles,
                     void *d_sym, int sym_bytes, uint8_t *d_states, hipStream_t st)
{
    const int N = tb.N, emit = tb.emit;
    const char *lds_env = std::getenv("IMC_SAMPLE_LDS");            // 0: every table read from global memory (A/B measurements)
    const bool lds_allowed = !(lds_env && std::atoi(lds_env) == 0);
    const size_t trans_bytes = tb.transition_doubles() * sizeof(double), all_bytes = tb.cdf.size() * sizeof(double);
    const bool summary_lds = lds_allowed && trans_bytes <= LDS_BUDGET;
    const bool emit_lds = lds_allowed && all_bytes <= SMP_EMIT_TABLE_LDS;

    DevBuf<double> d_tab;
    DevBuf<uint8_t> d_summ, d_enter;
    HIP_TRY(d_tab.alloc(all_bytes));
    HIP_TRY(d_summ.alloc((size_t)ntiles * N));
    HIP_TRY(d_enter.alloc(ntiles));
    HIP_TRY(hipMemcpyAsync(d_tab.get(), tb.cdf.data(), all_bytes, hipMemcpyHostToDevice, st));
    const SmpArgs a{d_tab.get(), N, emit, seed, tag, L, total, tile, ntiles};

    const bool timed = PhaseTimer::enabled();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto stamp = [&](int k) { if (timed && ev[k]) (void)hipEventRecord(ev[k], st); };
    if (timed)
        for (auto &e : ev) (void)hipEventCreate(&e);

    // summary: floor(64 / N) tiles per wavefront up to 64 states, ceil(N / 64) wavefronts per tile beyond
    const int sum_threads = summary_lds && trans_bytes >= SMP_SUMMARY_WIDE_FROM ? SMP_SUMMARY_WIDE_THREADS : SMP_THREADS;
    const uint64_t waves = N <= 64 ? ((uint64_t)ntiles + 64 / N - 1) / (64 / N) : (uint64_t)ntiles * ((N + 63) / 64);
    const uint64_t sum_blocks = (waves + sum_threads / 64 - 1) / (sum_threads / 64);
    if (sum_blocks >= (uint64_t)1 << 31) return fail(IMC_ERR_ARG, "imc_sample_device: too many tiles for one launch");
    stamp(0);
    if (summary_lds) {
        if (trans_bytes > 48 * 1024)
            if (int rc = allow_lds_budget(k_smp_summary<true>)) return rc;
        hipLaunchKernelGGL(k_smp_summary<true>, dim3((uint32_t)sum_blocks), dim3(sum_threads), trans_bytes, st, a, d_summ.get());
    } else
        hipLaunchKernelGGL(k_smp_summary<false>, dim3((uint32_t)sum_blocks), dim3(sum_threads), 0, st, a, d_summ.get());
    HIP_TRY(hipGetLastError());
    stamp(1);
    const int scan_threads = smp_scan_threads(N);
    hipLaunchKernelGGL(k_smp_scan, dim3(1), dim3(scan_threads), (size_t)2 * scan_threads * N, st, d_summ.get(), ntiles, N, d_enter.get());
    HIP_TRY(hipGetLastError());
    stamp(2);
    const dim3 emit_grid((ntiles + SMP_THREADS - 1) / SMP_THREADS);
    const size_t emit_lds_bytes = (emit_lds ? (all_bytes + 15) & ~(size_t)15 : 0) + smp_emit_stage_bytes(sym_bytes);
    if (sym_bytes == 1) {
        if (emit_lds) hipLaunchKernelGGL((k_smp_emit<true, uint8_t>), emit_grid, dim3(SMP_THREADS), emit_lds_bytes, st, a, d_enter.get(), (uint8_t *)d_sym, d_states);
        else hipLaunchKernelGGL((k_smp_emit<false, uint8_t>), emit_grid, dim3(SMP_THREADS), emit_lds_bytes, st, a, d_enter.get(), (uint8_t *)d_sym, d_states);
    } else {
        if (emit_lds) hipLaunchKernelGGL((k_smp_emit<true, uint16_t>), emit_grid, dim3(SMP_THREADS), emit_lds_bytes, st, a, d_enter.get(), (uint16_t *)d_sym, d_states);
        else hipLaunchKernelGGL((k_smp_emit<false, uint16_t>), emit_grid, dim3(SMP_THREADS), emit_lds_bytes, st, a, d_enter.get(), (uint16_t *)d_sym, d_states);
    }
    HIP_TRY(hipGetLastError());
    stamp(3);
    HIP_TRY(hipStreamSynchronize(st));     // the temporaries are freed on return
    if (timed) {
        float ms[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k)
            if (ev[k] && ev[k + 1]) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        std::fprintf(stderr, "[imc sample] %llu columns, %d states, tile %u (%u tiles): summary %.3f ms (%s table), scan %.3f ms, emit %.3f ms (%s tables)\n",
                     (unsigned long long)total, N, tile, ntiles, ms[0], summary_lds ? "LDS" : "global", ms[1], ms[2], emit_lds ? "LDS" : "global");
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    return IMC_OK;
}

}  // namespace
