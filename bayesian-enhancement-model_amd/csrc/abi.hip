// The library's error text (written by BEM_REQUIRE / bem_check_launch, one buffer per host thread) and its ABI version.
#include "bem_common.h"

thread_local char bem_err_buf[512] = "";
extern "C" const char* bem_last_error(void) { return bem_err_buf; }
extern "C" int bem_abi_version(void) { return 1; }
