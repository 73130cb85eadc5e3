// Error plumbing shared by every file that returns the C ABI's int codes: TRY propagates a non-zero code, API_BEGIN / API_END
// wrap the body of an extern "C" entry so that no C++ exception crosses the ABI (code 99, the message in mrisr_last_error).
#pragma once
#include <exception>
#include <string>

#include "common.h"

#define TRY(expr)            \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)
#define API_BEGIN try {
#define API_END                                                       \
    }                                                                 \
    catch (const std::exception& e) {                                 \
        ::mrisr::set_error(std::string("exception: ") + e.what());    \
        return 99;                                                    \
    }

namespace mrisr {
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
}  // namespace mrisr
