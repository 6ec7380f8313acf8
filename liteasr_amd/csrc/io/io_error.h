// The thread-local error text of libliteasr_io.so (lasr_io_last_error), shared by its sources.
#pragma once
#include <string>

namespace lasr_io {

inline thread_local std::string g_err;

inline int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

}  // namespace lasr_io
