// agt_knobs.h -- the debug knobs: environment variables that only AGT_DEBUG_KNOBS builds (make dbg / knobs) read, each once per site.
// In the product library a knob is its default, a constant, and the library reads no environment variable (tests/test_abi.py).
#pragma once
#ifdef AGT_DEBUG_KNOBS
#include <stdlib.h>
#define AGT_KNOB(name, def) ([] { static const long v_ = [] { const char* e_ = getenv(name); return e_ ? atol(e_) : (long)(def); }(); return v_; }())
#define AGT_KNOB_F(name, def) ([] { static const double v_ = [] { const char* e_ = getenv(name); return e_ ? atof(e_) : (double)(def); }(); return v_; }())
#else
#define AGT_KNOB(name, def) ((long)(def))
#define AGT_KNOB_F(name, def) ((double)(def))
#endif
