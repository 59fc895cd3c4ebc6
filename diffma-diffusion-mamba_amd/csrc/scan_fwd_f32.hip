// scan_fwd: f32 I/O instantiations (split per dtype so the library builds in parallel)
#include "scan_fwd_chunked.h"
namespace dm {
int scan_fwd_f32(const dm_scan_fwd_args& a, const dm_scan_fwd_args* second, hipStream_t st) { return dispatch_fwd<float>(a, second, st); }
bool scan_fwd_takes_two(const dm_scan_fwd_args& a) { return fwd_goes_chunked(a); }
}  // namespace dm

// tokens per segment of the chunk-parallel forward (scan_fwd_chunked.h) when a launch of this size -- without last_state, with
// arguments the family accepts -- takes it; 0 when it takes the sequential kernel.  The forward twin of dm_scan_bwd_launch_group_channels.
extern "C" int dm_scan_fwd_launch_segment(int nseq, int dim, int seqlen, int dstate, int flags) {
    return dm::fwd_chunked_segment(nseq, dim, seqlen, dstate, flags);
}
