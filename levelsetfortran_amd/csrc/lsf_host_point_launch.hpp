// lsf_host_point_launch.hpp -- what the host sides of the calls that work on points share (lsf_host_sample_points.hpp,
// lsf_host_cast_rays.hpp, lsf_host_points.hpp, lsf_host_reseed.hpp): the plan of a launch with one lane per point, the runtime flags
// as template arguments, and the finish of the per-block words.  Included by lsf_api.hip inside its anonymous namespace.
#pragma once

// One lane per item, `block` lanes per block, `npart` words per block in the S_PART slot (room for one block where count is 0,
// which only lsf_reseed_points allows: every other call refuses npts < 1).
struct PointPlan {
    int nblocks = 0;
    unsigned long long* part = nullptr;
};

int point_plan(PointPlan& p, size_t count, int block, int npart)
{
    p.nblocks = (int)((count + block - 1) / block);
    Buf& b = ctx().slot[S_PART];
    if (int rc = ws(b, (size_t)std::max(p.nblocks, 1) * npart * sizeof(unsigned long long))) return rc;
    p.part = (unsigned long long*)b.p;
    return LSF_OK;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the runtime values b0, b1, ...: the one place where flags become
// template arguments.  Every combination of the flags is instantiated; an f that has no kernel for one says so with if constexpr.
template <class F>
void with_flags(F&& f)
{
    f();
}
template <class F, class... B>
void with_flags(F&& f, bool b, B... rest)
{
    if (b)
        with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else
        with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// The finish of a launch whose blocks each left npart words in part: copies them home, synchronises the stream and combines them in
// block order into tot[0..npart) -- sums, and with last_is_max the last word as a maximum of bit patterns (integers: no order in the
// result).  Fills info, where one is given, with the sums.
int block_counts_finish(const unsigned long long* part, int nblocks, int npart, unsigned long long* tot, int64_t* info, hipStream_t st,
                        bool last_is_max = false)
{
    std::vector<unsigned long long> h((size_t)nblocks * npart);
    HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int nsum = npart - (last_is_max ? 1 : 0);
    for (int m = 0; m < npart; ++m) tot[m] = 0;
    for (int b = 0; b < nblocks; ++b) {
        for (int m = 0; m < nsum; ++m) tot[m] += h[(size_t)b * npart + m];
        if (last_is_max) tot[nsum] = std::max(tot[nsum], h[(size_t)b * npart + nsum]);
    }
    if (info)
        for (int m = 0; m < nsum; ++m) info[m] = (int64_t)tot[m];
    return LSF_OK;
}
