// The thread's error mark (csrc/err_mark.h) under several threads: every thread reads the text of its own failure, whatever another
// thread did on the same context in between.  Prints "bad N"; exit status 0 when N is 0.  Built plain and with -fsanitize=thread
// (tests/test_err_mark.py).
#include <stdio.h>
#include <string.h>
#include <condition_variable>
#include <mutex>
#include <thread>
#include "err_mark.h"

struct Barrier {
	std::mutex mu;
	std::condition_variable cv;
	const int n;
	int waiting = 0, round = 0;
	explicit Barrier(int n_) : n(n_) {}
	void wait()
	{
		std::unique_lock<std::mutex> lk(mu);
		const int r = round;
		if (++waiting == n) { waiting = 0, ++round; cv.notify_all(); }
		else cv.wait(lk, [&] { return round != r; });
	}
};

static int bad = 0;
static std::mutex bad_mu;
static void expect(bool ok, const char *what)
{
	if (ok) return;
	std::lock_guard<std::mutex> lk(bad_mu);
	++bad;
	fprintf(stderr, "failed: %s\n", what);
}
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

int main()
{
	int x = 0, y = 0; // two contexts: only their addresses matter
	const void *X = &x, *Y = &y;
	Barrier step(3);
	auto failing = [&](const char *text, int rc, bool first) {
		if (!first) step.wait(); // the second thread fails after the first has
		expect(gd_err_fail(X, rc, text) == rc, "gd_err_fail returns its code");
		if (first) step.wait();
		step.wait(); // both have failed on X
		expect(is(gd_err_text(X), text), "a thread reads its own text");
		expect(gd_err_text(Y) == nullptr, "a failure on X does not answer for Y");
		expect(gd_err_text(nullptr) == nullptr, "... nor for the null context");
		step.wait();
		// the null context: a writer opened without one
		expect(gd_err_fail(nullptr, -7, std::string("null: ") + text) == -7, "gd_err_fail(NULL)");
		expect(is(gd_err_text(nullptr), (std::string("null: ") + text).c_str()), "the null context reads its text");
		expect(gd_err_text(X) == nullptr, "the mark has moved off X");
		gd_err_clear();
		expect(gd_err_text(nullptr) == nullptr && gd_err_text(X) == nullptr, "gd_err_clear");
		expect(gd_err_fail(Y, -2, std::string("later: ") + text) == -2, "a later failure");
		expect(is(gd_err_text(Y), (std::string("later: ") + text).c_str()), "... replaces the text");
		step.wait();
	};
	std::thread a(failing, "read 7 record 0", -3, true), b(failing, "read 3 record 0", -4, false);
	std::thread c([&] { // never fails: null at every step
		for (int i = 0; i < 4; ++i) {
			expect(gd_err_text(X) == nullptr && gd_err_text(Y) == nullptr && gd_err_text(nullptr) == nullptr, "a thread that never failed reads null");
			step.wait();
		}
		expect(gd_err_text(X) == nullptr && gd_err_text(Y) == nullptr && gd_err_text(nullptr) == nullptr, "a thread that never failed reads null");
	});
	a.join(), b.join(), c.join();
	printf("bad %d\n", bad);
	return bad != 0;
}
