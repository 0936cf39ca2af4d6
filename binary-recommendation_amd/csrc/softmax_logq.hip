// L4: the log-Q forms of the in-batch softmax sweeps (candidate_sampling_probability of tfrs.tasks.Retrieval): the
// instantiations of softmax_kernel.h with InbatchLogqArgs.  The entries that launch them are in softmax.hip.
#include "softmax_kernel.h"

namespace br {

template <int MODE>
void launch_logq(const InbatchLogqArgs& a, int n_split, int id_type, bool emu, hipStream_t s) { launch_hard<MODE>(a, n_split, id_type, emu, s); }

template void launch_logq<MODE_THR>(const InbatchLogqArgs&, int, int, bool, hipStream_t);
template void launch_logq<MODE_LSE>(const InbatchLogqArgs&, int, int, bool, hipStream_t);
template void launch_logq<MODE_GRAD_R>(const InbatchLogqArgs&, int, int, bool, hipStream_t);
template void launch_logq<MODE_GRAD_C>(const InbatchLogqArgs&, int, int, bool, hipStream_t);
template void launch_logq<MODE_LSE_GRAD_R>(const InbatchLogqArgs&, int, int, bool, hipStream_t);

}  // namespace br
