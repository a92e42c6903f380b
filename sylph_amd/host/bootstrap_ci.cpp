// bootstrap_ci.cpp — the bootstrap confidence intervals of a sample's genomes as one batch: the resampling in one call on the device
// (sylph_bootstrap_counts, csrc/bootstrap.hip), everything behind the counts in inference.cpp's finish_ci, and the host's own loop for
// what the device declines or when SYLPH_HIP_BOOTSTRAP_DEVICE=0 asks for it.
#include <cstring>

#include "host_internal.hpp"

namespace sylph_host {

static_assert(sizeof(bootstrap_plan::Summary) == sizeof(sylph_bootstrap_summary), "the plan's summary is the ABI's");

BootstrapRoute bootstrap_route() {
    const char* e = getenv("SYLPH_HIP_BOOTSTRAP_DEVICE");
    if (!e || !*e || !strcmp(e, "1")) return BootstrapRoute::Device;
    if (!strcmp(e, "0")) return BootstrapRoute::Host;
    if (!strcmp(e, "only")) return BootstrapRoute::DeviceOnly;
    throw Error{1, std::string("SYLPH_HIP_BOOTSTRAP_DEVICE must be 0, 1 or only, not ") + e};
}

size_t bootstrap_batch(sylph_ctx* ctx, BootstrapRoute route, const ContainArgs& args, uint64_t k, const void* covs, uint32_t width,
                       const std::vector<CiItem>& items, uint64_t threads) {
    const size_t n = items.size();
    if (!n) return 0;
    std::vector<uint8_t> declined(n, 1);
    std::vector<bootstrap_plan::Summary> sums;
    if (route != BootstrapRoute::Host) {
        bool fits = n <= 0xFFFFFFFFull / BOOTSTRAP_ITERS;                    // (the call's counts are 32 bits wide)
        for (const auto& it : items) fits = fits && it.n_total <= 0xFFFFFFFFull;
        if (fits) {
            std::vector<uint64_t> cov_off(n + 1);
            std::vector<uint32_t> keep(n), n_total(n);
            for (size_t i = 0; i < n; i++) { cov_off[i] = items[i].cov_lo; keep[i] = (uint32_t)items[i].keep; n_total[i] = (uint32_t)items[i].n_total; }
            cov_off[n] = items.back().cov_hi;
            sums.resize(n * BOOTSTRAP_ITERS);
            hip_check(sylph_bootstrap_counts(ctx, covs, width, cov_off.data(), keep.data(), n_total.data(), (uint32_t)n, SYLPH_MEM_HOST, BOOTSTRAP_SEED,
                                             BOOTSTRAP_ITERS, reinterpret_cast<sylph_bootstrap_summary*>(sums.data()), declined.data()),
                      "sylph_bootstrap_counts");
        }
        if (route == BootstrapRoute::DeviceOnly)
            for (size_t i = 0; i < n; i++)
                if (declined[i]) throw Error{1, "SYLPH_HIP_BOOTSTRAP_DEVICE=only: the device declined the bootstrap of genome " + std::to_string(items[i].result->genome_index)};
    }
    parallel_for(n, threads, [&](size_t i) {
        const CiItem& it = items[i];
        if (!declined[i]) { finish_ci(&sums[i * BOOTSTRAP_ITERS], BOOTSTRAP_ITERS, it.n_total, (double)k, args, *it.result); return; }
        std::vector<uint32_t> kept(it.keep);
        for (size_t j = 0; j < it.keep; j++)
            kept[j] = width == 4 ? ((const uint32_t*)covs)[it.cov_lo + j] : width == 2 ? ((const uint16_t*)covs)[it.cov_lo + j] : ((const uint8_t*)covs)[it.cov_lo + j];
        bootstrap_host(kept.data(), it.keep, it.n_total, (double)k, args, *it.result);
    });
    size_t on_host = 0;
    for (uint8_t d : declined) on_host += d;
    return on_host;
}

}  // namespace sylph_host
