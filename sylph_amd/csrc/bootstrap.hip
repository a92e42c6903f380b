// bootstrap.hip — the resampling of bootstrap_interval (contain.rs:849-898) on the device: for every genome whose lambda was
// estimated, `iters` resamples of its n_total coverage values with replacement, each reduced to the five numbers ratio_lambda and
// ani_from_lambda read (bootstrap_plan.h Summary).  Lambda, ANI, the sort of the resamples and the percentiles stay on the host, in
// f64, in the code they always ran in: what comes back are counts.
//
// One workgroup per (item, resample): its 256 lanes stride over the n_total draws of the resample — draw j of a WyRand stream has the
// state seed + (j + 1) * WY_ADD, so a lane steps its state by 256 * WY_ADD and no draw waits for another — and count the drawn non-zero
// values in one LDS histogram per wave; zeros (most draws of a genome at low containment) are not counted, n_nonzero is the rest.
// Two ways from a drawn index to its value (sylph_ctx_set_option "bootstrap_shape"; profiles/bootstrap_device.txt has the comparison):
//   gather: covs[idx - n_zero], a load per non-zero draw;
//   table:  bound[v] = index of the first value >= v, made once per item by bootstrap_bounds_kernel and shared by its resamples; the
//           value is the run of compares idx >= bound[v + 1].  No load per draw, but a run as long as the value.
#include <algorithm>

#include "common.h"

#include "bootstrap_plan.h"

namespace sylph {
namespace {

using bootstrap_plan::BINS;
using bootstrap_plan::Summary;
static_assert(sizeof(Summary) == sizeof(sylph_bootstrap_summary) && sizeof(Summary) == 20, "the ABI's summary is the plan's");

constexpr int BOOT_TPB = 256, BOOT_WAVES = BOOT_TPB / 64;
enum BootShape : int { BOOT_GATHER = 0, BOOT_TABLE = 1 };

struct BootItem { uint64_t off; uint32_t keep, n_total; };   // covs[off .. off + keep) in elements of `width` bytes

__device__ __forceinline__ uint32_t load_cov(const void* covs, uint32_t width, uint64_t i) {
    return width == 4 ? ((const uint32_t*)covs)[i] : width == 2 ? (uint32_t)((const uint16_t*)covs)[i] : (uint32_t)((const uint8_t*)covs)[i];
}

// table shape: bound[item][v] = n_zero + number of kept values below v, for v < BINS
__global__ __launch_bounds__(64) void bootstrap_bounds_kernel(const void* __restrict__ covs, uint32_t width, const BootItem* __restrict__ items,
                                                              uint32_t* __restrict__ bound) {
    const BootItem im = items[blockIdx.x];
    const uint32_t v = threadIdx.x;
    uint32_t lo = 0, hi = im.keep;                      // first position whose value is >= v
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (load_cov(covs, width, im.off + mid) < v) lo = mid + 1;
        else hi = mid;
    }
    bound[(uint64_t)blockIdx.x * BINS + v] = (im.n_total - im.keep) + lo;
}

template <int SHAPE>
__global__ __launch_bounds__(BOOT_TPB) void bootstrap_kernel(const void* __restrict__ covs, uint32_t width, const BootItem* __restrict__ items,
                                                             const uint32_t* __restrict__ bound, uint64_t first_block, uint32_t iters, uint32_t bins,
                                                             uint64_t seed, Summary* __restrict__ out, uint32_t* __restrict__ declined) {
    __shared__ uint32_t hist[BOOT_WAVES][BINS];
    __shared__ uint32_t s_bound[BINS + 1];
    const uint64_t unit = first_block + blockIdx.x;                 // (item, resample)
    const uint32_t item = (uint32_t)(unit / iters), it = (uint32_t)(unit % iters);
    const uint32_t tid = threadIdx.x, wave = tid / 64;
    const BootItem im = items[item];
    const uint32_t n = im.n_total, n_zero = n - im.keep;
    // the values are ascending: the last kept one is the largest.  An item it does not fit the bins for declines as a whole.
    const uint32_t v_max = im.keep ? load_cov(covs, width, im.off + im.keep - 1) : 0u;
    if (v_max >= bins) {                                             // bins <= BINS
        if (tid == 0 && it == 0) declined[item] = 1u;
        return;
    }
    for (uint32_t i = tid; i < BOOT_WAVES * BINS; i += BOOT_TPB) (&hist[0][0])[i] = 0u;
    if (SHAPE == BOOT_TABLE && tid <= BINS) s_bound[tid] = tid < BINS ? bound[(uint64_t)item * BINS + tid] : 0xFFFFFFFFu;
    __syncthreads();
    // draw i of resample `it` is draw it * n + i of the item's stream (every resample makes n draws; the stream restarts per item)
    uint64_t state = bootstrap_plan::bootstrap_state(seed, (uint64_t)it * n + tid);
    constexpr uint64_t STEP = (uint64_t)BOOT_TPB * bootstrap_plan::WY_ADD;
    bool bad = false;
    uint64_t min_lo = ~0ull;                                         // smallest low half of r * n among those below n
#pragma unroll 4
    for (uint64_t i = tid; i < n; i += BOOT_TPB, state += STEP) {
        const uint64_t r = bootstrap_plan::wyrand_output(state);
        uint64_t lo;
        const uint32_t idx = bootstrap_plan::mul_64x32(r, n, lo);
        if (lo < n && lo < min_lo) min_lo = lo;                      // (n in 2^64 draws: Lemire's first test)
        if (idx < n_zero) continue;
        uint32_t v;
        if (SHAPE == BOOT_GATHER) {
            v = load_cov(covs, width, im.off + (idx - n_zero));
        } else {
            v = 0;
            while (idx >= s_bound[v + 1]) v++;                       // s_bound[BINS] = 2^32 - 1 > idx ends the run
        }
        if (v >= BINS) { bad = true; continue; }                     // (values that are not ascending: never counted out of bounds)
        if (v) atomicAdd(&hist[wave][v], 1u);
    }
    // fastrand draws again where lo < 2^64 mod n, which shifts every later draw of the stream: the item goes back to the host's loop
    if (min_lo != ~0ull && min_lo < (0 - (uint64_t)n) % n) bad = true;
    if (bad) declined[item] = 1u;
    __syncthreads();
    if (tid < BINS) {
        uint32_t c = hist[0][tid];
        for (int w = 1; w < BOOT_WAVES; w++) c += hist[w][tid];
        hist[0][tid] = c;
    }
    __syncthreads();
    if (tid == 0) out[unit] = bootstrap_plan::summary_of_histogram(hist[0], BINS);
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_bootstrap_counts(sylph_ctx* ctx, const void* covs, uint32_t cov_width, const uint64_t* cov_off, const uint32_t* keep,
                           const uint32_t* n_total, uint32_t n_items, int mem, uint64_t seed, uint32_t iters,
                           sylph_bootstrap_summary* out, uint8_t* declined) {
    return guarded([&] {
        SY_REQUIRE(ctx, "null context");
        SY_REQUIRE(cov_width == 1 || cov_width == 2 || cov_width == 4, "sylph_bootstrap_counts: coverage values of %u bytes", cov_width);
        SY_REQUIRE(iters != 0, "sylph_bootstrap_counts: no resamples asked for");
        SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE || mem == SYLPH_MEM_HOST_PINNED, "bad mem");
        if (!n_items) return;
        SY_REQUIRE(cov_off && keep && n_total && out && declined, "null argument");
        uint64_t kept_total = 0;
        for (uint32_t i = 0; i < n_items; i++) {
            SY_REQUIRE(cov_off[i] <= cov_off[i + 1], "sylph_bootstrap_counts: cov_off decreases at item %u", i);
            SY_REQUIRE(n_total[i] != 0, "sylph_bootstrap_counts: item %u has no values to draw from", i);
            SY_REQUIRE(keep[i] <= n_total[i], "sylph_bootstrap_counts: item %u keeps %u of %u values", i, keep[i], n_total[i]);
            SY_REQUIRE(keep[i] <= cov_off[i + 1] - cov_off[i], "sylph_bootstrap_counts: item %u keeps %u values of a row of %llu", i, keep[i],
                       (unsigned long long)(cov_off[i + 1] - cov_off[i]));
            kept_total += keep[i];
        }
        SY_REQUIRE(covs || kept_total == 0, "null argument");
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        const bool device_covs = mem == SYLPH_MEM_DEVICE;
        // host values: only the kept prefixes travel, side by side
        std::vector<BootItem> items(n_items);
        std::vector<uint8_t> packed;
        if (!device_covs) packed.resize(kept_total * cov_width);
        uint64_t at = 0;
        for (uint32_t i = 0; i < n_items; i++) {
            items[i] = BootItem{device_covs ? cov_off[i] : at, keep[i], n_total[i]};
            if (!device_covs && keep[i]) memcpy(packed.data() + at * cov_width, (const uint8_t*)covs + cov_off[i] * cov_width, (size_t)keep[i] * cov_width);
            at += keep[i];
        }
        const uint64_t units = (uint64_t)n_items * iters;
        DevBuf d_items(ctx), d_covs(ctx), d_out(ctx), d_decl(ctx), d_bound(ctx);
        d_items.reserve(items.size() * sizeof(BootItem));
        d_out.reserve(units * sizeof(Summary));
        d_decl.reserve((size_t)n_items * 4);
        ctx->h2d(d_items.p, items.data(), items.size() * sizeof(BootItem));
        const void* cv = covs;
        if (!device_covs) {
            d_covs.reserve(packed.size() + 16);
            ctx->h2d(d_covs.p, packed.data(), packed.size());
            cv = d_covs.p;
        }
        SY_HIP(hipMemsetAsync(d_decl.p, 0, (size_t)n_items * 4, ctx->stream));
        {
            ScopedKernelTimer t(ctx, "bootstrap");
            const bool table = ctx->bootstrap_shape == BOOT_TABLE;
            const uint32_t bins = std::min<uint32_t>(ctx->bootstrap_bins, BINS);
            if (table) {
                d_bound.reserve((size_t)n_items * BINS * 4);
                hipLaunchKernelGGL(bootstrap_bounds_kernel, dim3(n_items), dim3(BINS), 0, ctx->stream, cv, cov_width, d_items.as<BootItem>(),
                                   d_bound.as<uint32_t>());
            }
            constexpr uint64_t MAX_GRID = 1u << 30;
            for (uint64_t first = 0; first < units; first += MAX_GRID) {
                const uint32_t grid = (uint32_t)std::min<uint64_t>(MAX_GRID, units - first);
                if (table)
                    hipLaunchKernelGGL(bootstrap_kernel<BOOT_TABLE>, dim3(grid), dim3(BOOT_TPB), 0, ctx->stream, cv, cov_width, d_items.as<BootItem>(),
                                       d_bound.as<uint32_t>(), first, iters, bins, seed, d_out.as<Summary>(), d_decl.as<uint32_t>());
                else
                    hipLaunchKernelGGL(bootstrap_kernel<BOOT_GATHER>, dim3(grid), dim3(BOOT_TPB), 0, ctx->stream, cv, cov_width, d_items.as<BootItem>(),
                                       (const uint32_t*)nullptr, first, iters, bins, seed, d_out.as<Summary>(), d_decl.as<uint32_t>());
            }
            SY_HIP(hipGetLastError());
        }
        std::vector<uint32_t> decl(n_items);
        ctx->d2h(out, d_out.p, units * sizeof(Summary));
        ctx->d2h(decl.data(), d_decl.p, (size_t)n_items * 4);
        for (uint32_t i = 0; i < n_items; i++) declined[i] = decl[i] ? 1 : 0;
    });
}

}  // extern "C"
