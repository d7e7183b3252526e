// lsf_host_stop.hpp -- the device-side stop flag of the iterative calls and the host's side of it: one driver for the Jacobi reinit, the
// reinit on the band, the field advection and both min/max executors.  (The exact-GS drivers, lsf_host_gs.hpp and lsf_gs_slabs.hpp, keep
// their own: there the verdict is tied to the batch planning.)  Included by lsf_api.hip inside its anonymous namespace.
// A loop enqueues its sweeps ahead of the device; the last kernel of a sweep (k_finish, k_advect_finish) gives the verdict
// and every kernel enqueued past a stop returns at once.  The host looks every CHECK_EVERY sweeps, so at most CHECK_EVERY - 1 empty
// sweeps are enqueued past the verdict, and COUNT -- never the host's loop counter -- says which buffer holds the result.
#pragma once

// The control words are CtlWord (lsf_kernels.hpp): the kernels and this driver address them by the same names.
struct StopLoop {
    int* ctl = nullptr;        // device: the control words
    double* d_trace = nullptr; // device: one value per completed sweep, written by the finish kernel
    int trace_entries = 0;     // ... which is told to write at most this many
    int host[CTL_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0}; // the words as last read
    hipStream_t st = nullptr;
    int rc = LSF_OK; // a failed read inside look(): the loop is left and finish() returns it

    // sizes S_CTL and S_TRACE and clears the control words (in stream order: after whatever the caller has enqueued so far)
    int begin(Ctx& c, int entries, hipStream_t stream)
    {
        int r;
        if ((r = ws(c.slot[S_CTL], CTL_BYTES)) || (r = ws(c.slot[S_TRACE], (size_t)std::max(entries, 1) * sizeof(double)))) return r;
        ctl = (int*)c.slot[S_CTL].p, d_trace = (double*)c.slot[S_TRACE].p, trace_entries = entries, st = stream;
        HIPCHK(hipMemsetAsync(ctl, 0, CTL_BYTES, st));
        return LSF_OK;
    }
    int read()
    {
        HIPCHK(hipMemcpyAsync(host, ctl, sizeof host, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return LSF_OK;
    }
    // after sweep s (0-based) of `total` has been enqueued: is a look at the device due?  Every CHECK_EVERY sweeps, or when the caller
    // says so, but never after the last sweep: finish() reads the words anyway.
    static bool due(int s, int total, bool also_now = false) { return ((s + 1) % CHECK_EVERY == 0 || also_now) && s + 1 < total; }
    // reads the words (waits for the device); true = leave the loop
    bool look() { return (rc = read()) != LSF_OK || host[CTL_STOP] || host[CTL_UNCERT]; }
    bool poll(int s, int total) { return due(s, total) && look(); }
    // behind the loop, however it was left: launch errors, the final words
    int finish()
    {
        if (rc) return rc;
        HIPCHK(hipGetLastError());
        return read();
    }
    int count() const { return host[CTL_COUNT]; }
    bool stopped() const { return host[CTL_STOP] != 0; }
    // the caller has put the result in place: the trace (at most `cap` entries) and the count go home, NaN becomes the call's error
    int verdict(double* trace_out, int cap, int* done, const std::string& nan_msg)
    {
        const int cnt = count();
        if (trace_out && cap > 0 && cnt > 0)
            HIPCHK(hipMemcpyAsync(trace_out, d_trace, sizeof(double) * (size_t)std::min(cnt, cap), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (done) *done = cnt;
        return host[CTL_NAN] ? fail(LSF_ERR_NAN, nan_msg) : LSF_OK;
    }
};

// The RMS: the partials summed in a fixed order by one block -- through 256 slice sums where the caller has room for them (part2) and
// there are more than `slices_above` -- then the verdict (k_finish)
void reduce_finish(const double* part, long n, double* part2, double den, double tol, const StopLoop& stop, long slices_above = 16384)
{
    if (part2 && n > slices_above) {
        hipLaunchKernelGGL(k_reduce_slices, dim3(256), dim3(256), 0, stop.st, part, n, part2);
        part = part2, n = 256L;
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(RED_T), 0, stop.st, part, n, den, tol, stop.d_trace, stop.trace_entries, stop.ctl);
}
