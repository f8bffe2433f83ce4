// http_phases.h — the HTTP compiler's back end (http_phases.cc) as seen by its
// front end (http_compile.cc).  Host only: no device unit includes this.
#pragma once
#include "l7m_internal.h"

namespace l7m {

// One compile of flattened rules under a port-entry plan: the phases of
// http_phases.cc in order.  no_alit: fields whose literal-anchored scan is
// turned off (their patterns stay search groups); set by
// compile_http_alit_fallback when a field's bucket table does not fit the LDS
// budget.  *alit_over receives such a field.
CompileResult compile_http_core(const l7m_http_rule* rules, size_t n, const PolicyPlan& plan, const l7m_opts& opts,
                                uint64_t no_alit, uint32_t* alit_over);

}  // namespace l7m
