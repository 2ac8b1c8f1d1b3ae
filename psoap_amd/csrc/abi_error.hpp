// abi_error.hpp -- the error channel of the C ABI (include/psoap_gp.h): the calling thread's last message, the macro that
// sets it and returns 2, and psoap_last_error.  No HIP header.
#pragma once
#include <string>

static thread_local std::string g_err;

#define FAIL(msg)                \
    do {                         \
        g_err = std::string(msg); \
        return 2;                \
    } while (0)

extern "C" const char* psoap_last_error(void) { return g_err.c_str(); }
