// vss_actuate_build_info.cpp — the source stamp of libvss_actuate.so (include/vss_actuate.h vss_actuate_source_hash).
// VSS_ACTUATE_SOURCE_HASH is the first 16 hex digits of sha256 over the files of this directory's Makefile's STAMPED
// line, in its order, computed at build time; vss_amd/actuate.py recomputes it from the tree and refuses a library
// built from other sources, as vss_amd/_native.py does for the core library.
#include "../../../include/vss_actuate.h"

#ifndef VSS_ACTUATE_SOURCE_HASH
#error "VSS_ACTUATE_SOURCE_HASH must be defined by the build (csrc/actuate/Makefile)"
#endif

extern "C" const char* vss_actuate_source_hash(void) { return VSS_ACTUATE_SOURCE_HASH; }
