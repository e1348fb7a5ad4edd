// CPU: the rounds of the drain launches over a pending list (ksw_plan.h: gd_drain_rounds, gd_drain_replay; the claim's own test is
// gd_claim_fits of ksw_wave_core.h, which the kernel uses).  For a set of pending boxes and an arena: the number of rounds the host
// enqueues, and the claims replayed in several orders of arrival, checked by brute force -- every box is served exactly once, the slots
// of a round are pairwise disjoint and inside the arena, and no more rounds are used or enqueued than gd_drain_launches allows for the
// same set.  Status 1 at the first property that does not hold; one line per case for tests/test_drain_rounds.py.
#define __host__
#define __device__
#include <stdio.h>
#include <stdlib.h>
#include <numeric>
#include <random>
#include "ksw_plan.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d, case %s)\n", #c, __LINE__, name); exit(1); } } while (0)

// the rounds one order of arrival uses; checks the replay's answer by brute force
static int check_order(const char *name, const std::vector<uint32_t> &units, size_t arena, int n_rounds)
{
	std::vector<int32_t> round;
	std::vector<uint32_t> off;
	const size_t left = gd_drain_replay(units, arena, n_rounds, round, off);
	CHECK(left == 0);
	CHECK(round.size() == units.size() && off.size() == units.size());
	int used = 0;
	std::vector<int> served(units.size(), 0);
	for (int k = 1; k <= n_rounds; ++k)
		for (size_t i = 0; i < units.size(); ++i) {
			if (round[i] != k) continue;
			++served[i], used = k;
			CHECK(((size_t)off[i] + units[i]) * 256 <= arena); // inside the arena
			for (size_t j = i + 1; j < units.size(); ++j) // disjoint from every other box of the round
				if (round[j] == k) CHECK((size_t)off[i] + units[i] <= off[j] || (size_t)off[j] + units[j] <= off[i]);
		}
	for (size_t i = 0; i < units.size(); ++i) CHECK(served[i] == 1 && round[i] >= 1 && round[i] <= n_rounds);
	return used;
}

// a pending set inside a batch whose planner summed batch_total / batch_max over every box that could have been pending
static void check_set(const char *name, const std::vector<uint32_t> &units, size_t arena, size_t batch_n, size_t batch_total, size_t batch_max, std::mt19937_64 &rng)
{
	size_t total = 0, largest = 0;
	for (uint32_t u : units) total += (size_t)u * 256, largest = std::max(largest, (size_t)u * 256);
	CHECK(total <= batch_total && largest <= batch_max && units.size() <= batch_n && arena >= batch_max);
	const int allowed = gd_drain_launches(units.size(), total, largest, arena);           // ... for this very set
	const int planned = gd_drain_launches(batch_n, batch_total, batch_max, arena);        // the batch's n_drain: its claim counters
	const int own = gd_drain_rounds(GdDrainSet{units.size(), total, largest}, arena);     // the host knows the set's own sums
	const int n_rounds = gd_drain_rounds(GdDrainSet{units.size(), batch_total, batch_max}, arena); // the host knows the batch's only
	CHECK(own <= allowed && own <= n_rounds && n_rounds <= planned);
	CHECK((units.empty() && n_rounds == 0) || (!units.empty() && own >= 1));
	int used_max = 0;
	std::vector<uint32_t> v = units;
	for (int order = 0; order < 6; ++order) {
		if (order == 1) std::sort(v.begin(), v.end());
		else if (order == 2) std::sort(v.begin(), v.end(), std::greater<uint32_t>());
		else if (order > 2) std::shuffle(v.begin(), v.end(), rng);
		const int used = check_order(name, v, arena, own); // (the tighter count already serves every order)
		CHECK(used <= allowed);
		CHECK(check_order(name, v, arena, n_rounds) == used); // more rounds enqueued: the same claims, the rest find nothing pending
		used_max = std::max(used_max, used);
	}
	printf("%s n=%zu arena=%zu rounds=%d own=%d used=%d allowed=%d planned=%d\n", name, units.size(), arena, n_rounds, own, used_max, allowed, planned);
}

int main()
{
	std::mt19937_64 rng(20261020);
	{ // nothing pending in a batch of 100 boxes
		check_set("none", {}, (size_t)200 << 8, 100, (size_t)100 * 200 * 256, (size_t)200 << 8, rng);
	}
	{ // one box, the arena exactly its size
		check_set("one", {123}, (size_t)123 << 8, 1, (size_t)123 << 8, (size_t)123 << 8, rng);
	}
	{ // every box of the batch pending
		std::vector<uint32_t> u;
		for (int i = 0; i < 40; ++i) u.push_back((uint32_t)(1 + rng() % 256));
		size_t total = 0, largest = 0;
		for (uint32_t x : u) total += (size_t)x << 8, largest = std::max(largest, (size_t)x << 8);
		check_set("all", u, largest + (total - largest) / 3, u.size(), total, largest, rng);
	}
	{ // equal boxes in an arena of one: a box per round
		const char *name = "one_per_round";
		std::vector<uint32_t> u(17, 256);
		check_set(name, u, (size_t)256 << 8, u.size(), (size_t)17 * 256 * 256, (size_t)256 << 8, rng);
		CHECK(gd_drain_rounds(GdDrainSet{17, (size_t)17 * 256 * 256, (size_t)256 << 8}, (size_t)256 << 8) == 17);
		CHECK(check_order(name, u, (size_t)256 << 8, 17) == 17);
	}
	for (int draw = 0; draw < 200; ++draw) { // up to 64 sizes of 256 B .. 64 KB, the arena between the largest and the total; the set alone, and inside a larger batch
		char name[32];
		snprintf(name, sizeof name, "draw%d", draw);
		std::vector<uint32_t> u((size_t)(1 + rng() % 64));
		for (uint32_t &x : u) x = (uint32_t)(1 + rng() % 256);
		size_t total = 0, largest = 0;
		for (uint32_t x : u) total += (size_t)x << 8, largest = std::max(largest, (size_t)x << 8);
		size_t batch_n = u.size(), batch_total = total, batch_max = largest;
		if (draw & 1) { // the pending set is a part of the batch
			const size_t more = 1 + rng() % 64;
			for (size_t i = 0; i < more; ++i) {
				const size_t x = (size_t)(1 + rng() % 256) << 8;
				++batch_n, batch_total += x, batch_max = std::max(batch_max, x);
			}
		}
		const size_t lo = batch_max, hi = std::max(batch_max, total);
		const size_t arena = lo + ((rng() % ((hi - lo) / 256 + 1)) << 8);
		check_set(name, u, arena, batch_n, batch_total, batch_max, rng);
	}
	printf("ok\n");
	return 0;
}
