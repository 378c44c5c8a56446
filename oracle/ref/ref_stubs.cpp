// Definitions for the reference symbols that the driver's link needs but never calls: the GPU factory (the
// driver runs the CPU back end) and the netCDF reader's constructor, destructor and readers (the driver fills
// the objects itself).  The Makefile lists those undefined symbols from the compiled objects into
// ref_stub_symbols.inc, one MOPS_REF_STUB(mangled name) per line; each becomes an alias of the function below.
#include <cstdio>
#include <cstdlib>

extern "C" {

void mops_ref_unreachable()
{
    std::fputs("mops_ref_driver: a reference function outside the CPU path was called\n", stderr);
    std::abort();
}

#define MOPS_REF_STUB(sym) void sym() __attribute__((alias("mops_ref_unreachable")));
#include "ref_stub_symbols.inc"
}
