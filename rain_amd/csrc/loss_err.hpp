// loss_err.hpp — the last-error slot of librain_loss.so (rl_last_error, include/rain_loss.h), shared
// by the library's sources.  Defined in loss.hip.
#pragma once

#include <string>

namespace rl_detail {
extern thread_local std::string g_err;
}
