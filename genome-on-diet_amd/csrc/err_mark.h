// The text of a failure that must not go through gdiet_ctx::err: the side lanes (difference strings, the reader's device mode, BGZF,
// BAM) fail on writer and reader threads while a mapping thread may be writing err.  One mark per thread: gdiet_hip_strerror hands the
// text to the thread whose call failed, until that thread's next call that clears it.  Host-only: the context is an address to compare,
// NULL included (a BGZF writer opened without a context reports through gdiet_hip_strerror(NULL)).
#pragma once
#include <string>

struct GdErrMark { bool set = false; const void *on = nullptr; std::string text; };
static inline GdErrMark &gd_err_mark()
{
	static thread_local GdErrMark m;
	return m;
}
static inline void gd_err_clear() { gd_err_mark().set = false; }
static inline int gd_err_fail(const void *on, int rc, const std::string &text)
{
	GdErrMark &m = gd_err_mark();
	m.text = text, m.on = on, m.set = true;
	return rc;
}
static inline const char *gd_err_text(const void *on)
{
	const GdErrMark &m = gd_err_mark();
	return m.set && m.on == on ? m.text.c_str() : nullptr;
}
