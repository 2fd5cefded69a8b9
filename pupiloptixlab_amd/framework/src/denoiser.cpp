// denoiser.cpp — the out-of-line part of Pupil::optix::Denoiser (pupil/denoiser.h).
#include "pupil/denoiser.h"

namespace Pupil::optix {

void Denoiser::ResetHistory() noexcept {
    if (m_denoiser) (void)pupil_denoiser_reset_history(m_denoiser);
}

}  // namespace Pupil::optix
