// ps_error.h -- what every entry point of the library throws.
#pragma once
#include <stdexcept>

namespace ps {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

}  // namespace ps
