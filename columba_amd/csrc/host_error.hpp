// How every translation unit of the library reports an error (no HIP: the host-only units include it too)
#pragma once
#include <string>

namespace cmb {
// sets the calling thread's cmb_last_error and returns `code` (columba_amd.hip)
int failWith(int code, const std::string& msg);
} // namespace cmb
