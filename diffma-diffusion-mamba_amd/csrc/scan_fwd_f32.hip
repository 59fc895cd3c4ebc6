// scan_fwd: f32 I/O instantiations (split per dtype so the library builds in parallel)
#include "scan_fwd_chunked.h"
namespace dm {
int scan_fwd_f32(const dm_scan_fwd_args& a, const dm_scan_fwd_args* second, hipStream_t st) { return dispatch_fwd<float>(a, second, st); }
bool scan_fwd_takes_two(const dm_scan_fwd_args& a) { return fwd_goes_chunked(a); }
}  // namespace dm
