// lsf_host_point_launch.hpp -- what the host sides of the calls that work on points share (lsf_host_sample_points.hpp,
// lsf_host_cast_rays.hpp, lsf_host_points.hpp, lsf_host_reseed.hpp): the plan of a launch with one lane per point.  The runtime flags
// as template arguments (with_flags) and the finish of the per-block words (block_counts_finish) are shared with the band calls and
// live in lsf_host_band.hpp.  Included by lsf_api.hip inside its anonymous namespace.
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
