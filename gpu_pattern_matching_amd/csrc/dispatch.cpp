// The dispatcher behind every scan entry point: which pipeline a batch gets, launch groups, the
// HIP-graph cache and in-line timing.  Host code only -- the three pipelines enqueue their own
// kernels behind chain.h (scan.hip), sparse.h (sparse.hip) and lds_walk.h (lds_walk.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "acm_internal.h"
#include "chain.h"
#include "device_dfa.h"
#include "lds_walk.h"
#include "sparse.h"

namespace {

// Which pipeline the next batch gets.  Tiny texts are not worth the sieve's tables.  In AUTO
// mode the choice adapts: the sparse pipeline is exact on any text but slow on one that is dense
// in matches or in flagged samples (its emit kernel counts such batches, sparse.hip), so when
// half of the last 16 sparse batches were dense the next 64 go to the chain pipeline, then the
// sparse one is tried again -- for 4 batches; if half of those are dense again the chain
// pipeline gets four times as many batches as last time (up to 4096), and so on until a look
// finds the text quiet.
bool pick_sparse(const acm_dfa *d, size_t n)
{
	if (!d->sparse_ok || d->scan_mode == ACM_SCAN_MODE_CHAIN || n < 64)
		return false;
	if (d->scan_mode != ACM_SCAN_MODE_AUTO || !d->h_giveups)
		return true;
	uint32_t hold = d->chain_hold.load(std::memory_order_relaxed);
	while (hold > 0)
		if (d->chain_hold.compare_exchange_weak(hold, hold - 1, std::memory_order_relaxed))
			return false;
	const uint32_t count = d->sparse_batches.fetch_add(1, std::memory_order_relaxed) + 1;
	const uint32_t window = d->auto_window.load(std::memory_order_relaxed);
	if (count >= window) {
		d->sparse_batches.store(0, std::memory_order_relaxed);
		const uint32_t seen = *(volatile uint32_t *)d->h_giveups;   // written by k_sieve_emit, may lag
		const uint32_t before = d->giveups_seen.exchange(seen, std::memory_order_relaxed);
		if (seen - before >= window / 2) {
			const uint32_t stay = d->auto_next_hold.load(std::memory_order_relaxed);
			d->chain_hold.store(stay, std::memory_order_relaxed);
			d->auto_next_hold.store(std::min<uint32_t>(stay * 4, 4096u), std::memory_order_relaxed);
			d->auto_window.store(4, std::memory_order_relaxed);
		} else {
			d->auto_next_hold.store(64, std::memory_order_relaxed);
			d->auto_window.store(16, std::memory_order_relaxed);
		}
	}
	return true;
}

// the chain pipeline's LDS-resident form takes launch groups too (lds_walk.hip)
bool lds_path(const acm_dfa *d, bool sparse, size_t n) { return !sparse && d->lds_ok && d->use_halo && n > 0; }
uint32_t max_group_limit() { return std::min(acm::sparse_max_group(), acm::lds_walk_max_group()); }

// The four events that time one launch, or one launch group: before the first kernel, behind the
// first stage, behind the second, behind the last.  take() gets them from d->profile_pool (recycled:
// no create/destroy in a timed loop), commit() hands them to acm_scan_profile_read, and whatever was
// taken and not committed goes back to the pool.  Not taken: four null events, commit() does nothing.
class TimingEvents {
public:
	explicit TimingEvents(const acm_dfa *d) : d_(d) {}
	~TimingEvents() { move_to(d_->profile_pool); }
	int take()
	{
		std::lock_guard<std::mutex> lock(d_->profile_mutex);
		for (auto &e : ev_) {
			if (d_->profile_pool.empty()) {
				ACM_HIP_TRY(hipEventCreate(&e));
				continue;
			}
			e = (hipEvent_t)d_->profile_pool.back();
			d_->profile_pool.pop_back();
		}
		return ACM_OK;
	}
	void commit() { move_to(d_->profile_events); }
	hipEvent_t operator[](int k) const { return ev_[k]; }

private:
	void move_to(std::vector<void *> &list)
	{
		if (!ev_[0])   // (taken front to back)
			return;
		std::lock_guard<std::mutex> lock(d_->profile_mutex);
		for (auto &e : ev_) {
			if (e)
				list.push_back((void *)e);
			e = nullptr;
		}
	}
	const acm_dfa *d_;
	hipEvent_t ev_[4] = { nullptr, nullptr, nullptr, nullptr };
};

int record(hipEvent_t e, hipStream_t s)
{
	if (e)
		ACM_HIP_TRY(hipEventRecord(e, s));
	return ACM_OK;
}

// What a batch comes to once its arguments have been checked: nothing of it touches the stream.
enum class Path { Empty, Sieve, LdsWalk, Chain };
struct Plan {
	Path path;
	acm::ScanLayout l;
	uint32_t init_dev;   // device id of init_state
	uint32_t *misc;
};

// grouped: the batch is a member of a launch group (acm_scan_batches_async)
int plan_batch(const acm_dfa *d, const acm_scan_batch *b, bool sparse, bool grouped, Plan *p)
{
	if (!d || !b->d_pat_plane || !b->d_off_plane || b->plane_capacity < 2 || (b->n && !b->d_text))
		return acm::fail(ACM_ERR_ARG, "acm_scan_async: bad arguments");
	if (b->n > 0x7FFFFFEFul)
		return acm::fail(ACM_ERR_LIMIT, "acm_scan_async: %zu bytes exceed the 2 GiB buffer limit", b->n);
	if (((uintptr_t)b->d_text & 15) != 0)
		return acm::fail(ACM_ERR_ARG, "acm_scan_async: text must be 16-byte aligned");
	if (b->report != ACM_REPORT_HEAD && b->report != ACM_REPORT_STATE)
		return acm::fail(ACM_ERR_ARG, "acm_scan_batch_async: report %d is not an ACM_REPORT_* value", b->report);
	if (b->halo > b->n || b->offset_shift < INT32_MIN || b->offset_shift > INT32_MAX ||
	    (long)b->n + b->offset_shift > (long)INT32_MAX)
		return acm::fail(ACM_ERR_ARG, "acm_scan_shard_async: halo/offset_shift out of range");
	if (b->d_init_plane && b->init_plane_capacity < 2)
		return acm::fail(ACM_ERR_ARG, "acm_scan_batch_async: d_init_plane needs the capacity its scan was given");
	if (b->init_state < 0 || (uint64_t)b->init_state >= d->num_states)
		return acm::fail(ACM_ERR_ARG, "acm_scan_async: init_state %ld is not a state", b->init_state);
	const acm::ScanLayout &l = p->l = acm::scan_layout(d, b->n);
	if (!b->d_workspace || b->workspace_bytes < l.total)
		return acm::fail(ACM_ERR_ARG, "acm_scan_async: workspace %zu B < required %zu B", b->workspace_bytes, l.total);
	if (b->d_init_plane && grouped)   // (groupable() keeps such batches out of groups)
		return acm::fail(ACM_ERR_ARG, "acm_scan_batches_async: a batch with d_init_plane cannot join a launch group");
	p->path = b->n == 0 ? Path::Empty : sparse ? Path::Sieve : lds_path(d, sparse, b->n) ? Path::LdsWalk : Path::Chain;
	if (p->path == Path::LdsWalk) {   // the automaton fits the LDS whole: walk + scatter of lds_walk.hip
		size_t stage_words, cnt_bytes, tile_words;
		acm::lds_walk_needs(d, b->n, &stage_words, &cnt_bytes, &tile_words);
		if (stage_words * 4 > l.stage2 - l.stage1 || cnt_bytes > l.off - l.cnt || tile_words * 4 > l.wave_cnt1 - l.off)
			return acm::fail(ACM_ERR_ARG, "acm_scan_async: workspace layout too small for the LDS walk");
	}
	p->init_dev = d->ref2dev[(size_t)b->init_state];
	p->misc = (uint32_t *)((char *)b->d_workspace + l.misc);
	return ACM_OK;
}

// init_code_ptr: null, or where carry_init_enqueue left the state to start in
acm::LdsJob lds_job(const acm_scan_batch *b, const Plan &p, const uint32_t *init_code_ptr)
{
	char *ws = (char *)b->d_workspace;
	return { b, (uint32_t *)(ws + p.l.stage1), (uint8_t *)(ws + p.l.cnt), (uint32_t *)(ws + p.l.off), p.misc, init_code_ptr };
}

// one batch with its launches to itself
int enqueue_batch(const acm_dfa *d, const acm_scan_batch *b, bool sparse)
{
	Plan p;
	int rc = plan_batch(d, b, sparse, false, &p);
	if (rc != ACM_OK)
		return rc;
	hipStream_t s = (hipStream_t)b->stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	TimingEvents ev(d);
	if ((d->profile || b->profile) && (rc = ev.take()) != ACM_OK)
		return rc;
	if (b->wait_before_walk)
		ACM_HIP_TRY(hipStreamWaitEvent(s, (hipEvent_t)b->wait_before_walk, 0));
	if ((rc = record(ev[0], s)) != ACM_OK)
		return rc;
	const bool carried = b->d_init_plane != nullptr;   // the state to start in comes from another scan's planes, on the device
	if (carried && (rc = acm::carry_init_enqueue(d, b, p.misc, s)) != ACM_OK)
		return rc;
	const uint32_t *init_dev_ptr = carried ? p.misc + acm::kMiscInitDev : nullptr;
	const uint32_t *init_code_ptr = carried ? p.misc + acm::kMiscInitCode : nullptr;
	const hipEvent_t rec = (hipEvent_t)b->record_after_walk;
	acm::LdsJob job;
	switch (p.path) {
	case Path::Empty:   // (no walk: the batch behind this one waits for nothing older than this point)
		rc = acm::empty_scan_enqueue(d, b, p.l, p.init_dev, init_dev_ptr, s);
		for (hipEvent_t e : { rec, ev[1], ev[2] })
			if (rc == ACM_OK)
				rc = record(e, s);
		break;
	case Path::LdsWalk:
		job = lds_job(b, p, init_code_ptr);
		rc = acm::lds_walk_enqueue(d, &job, 1, s, ev[1], rec);
		if (rc == ACM_OK)
			rc = record(ev[2], s);   // (the walk is the first stage, there is no second)
		break;
	case Path::Sieve:   // three kernels of its own; it always produces the planes
		rc = acm::sparse_scan_enqueue(d, b, p.init_dev, init_dev_ptr, (char *)b->d_workspace + p.l.sparse,
		    p.misc + acm::kMiscPath, s, ev[1], ev[2]);
		if (rc == ACM_OK)
			rc = record(rec, s);
		break;
	case Path::Chain:
		rc = acm::chain_scan_enqueue(d, b, p.l, p.init_dev, init_dev_ptr, s, ev[1], ev[2]);
		break;
	}
	if (rc == ACM_OK)
		rc = record(ev[3], s);
	if (rc == ACM_OK)
		ev.commit();
	return rc;
}

// consecutive sparse batches of one size on one stream, each with its own workspace and planes,
// that wait for nothing and are not timed: one group for the sparse kernels
bool groupable(const acm_dfa *d, const acm_scan_batch &b)
{
	return !d->profile && !b.wait_before_walk && !b.record_after_walk && !b.d_init_plane && b.n > 0;
}

bool joins(const acm_scan_batch *const *group, uint32_t m, const acm_scan_batch &b)
{
	if (b.stream != group[0]->stream || b.n != group[0]->n || (b.profile != 0) != (group[0]->profile != 0))
		return false;   // (a group is timed as a whole or not at all)
	for (uint32_t i = 0; i < m; i++)
		if (b.d_workspace == group[i]->d_workspace || b.d_pat_plane == group[i]->d_pat_plane || b.d_off_plane == group[i]->d_off_plane)
			return false;
	return true;
}

// A launch group: m > 1 batches that groupable() and joins() let through, one set of kernels for all.
// Failure contract: "stops at the first batch that fails; the batches before it stay enqueued" --
// also inside a group: the members in front of the one that failed validation are launched (as a
// shorter group), the status of the failing one is returned.
int enqueue_group(const acm_dfa *d, const acm_scan_batch *const *group, uint32_t m, bool sparse)
{
	acm::SieveJob sj[32];
	acm::LdsJob lj[32];
	uint32_t good = 0;
	int first_bad = ACM_OK;
	for (; good < m; good++) {
		Plan p;
		first_bad = plan_batch(d, group[good], sparse, true, &p);
		if (first_bad != ACM_OK)
			break;
		if (sparse)
			sj[good] = { group[good], p.init_dev, nullptr, (char *)group[good]->d_workspace + p.l.sparse, p.misc + acm::kMiscPath };
		else
			lj[good] = lds_job(group[good], p, nullptr);
	}
	if (good == 0)
		return first_bad;
	hipStream_t s = (hipStream_t)group[0]->stream;
	ACM_HIP_TRY(hipSetDevice(d->device));
	TimingEvents ev(d);   // the group's kernels, timed like a single batch's
	int rc = group[0]->profile ? ev.take() : ACM_OK;
	if (rc == ACM_OK)
		rc = record(ev[0], s);
	if (rc == ACM_OK && sparse) {
		rc = acm::sparse_group_enqueue(d, sj, good, s, ev[1], ev[2]);
	} else if (rc == ACM_OK) {
		rc = acm::lds_walk_enqueue(d, lj, good, s, ev[1], nullptr);
		if (rc == ACM_OK)
			rc = record(ev[2], s);   // (the walk is the first stage, there is no second)
	}
	if (rc == ACM_OK)
		rc = record(ev[3], s);
	if (rc != ACM_OK)
		return rc;
	ev.commit();
	return first_bad;
}

// what a cached graph was captured for: every input of enqueue_batch except the stream
acm_dfa::GraphKey graph_key(const acm_dfa *d, const acm_scan_batch *b, bool sparse)
{
	acm_dfa::GraphKey k;
	memset(&k, 0, sizeof(k));   // (compared with memcmp)
	k.batch = *b;
	k.batch.stream = nullptr;
	k.mode = sparse ? ACM_SCAN_MODE_SPARSE : ACM_SCAN_MODE_CHAIN;
	k.chain_bytes = d->chain_bytes;
	k.chains_per_lane = d->chains_per_lane;
	return k;
}

}  // namespace

extern "C" int acm_scan_set_mode(acm_dfa *d, int mode)
{
	if (!d)
		return ACM_SCAN_MODE_CHAIN;
	if (mode == ACM_SCAN_MODE_AUTO || mode == ACM_SCAN_MODE_CHAIN || mode == ACM_SCAN_MODE_SPARSE)
		d->scan_mode = mode;
	return d->scan_mode;
}

extern "C" int acm_scan_sparse_eligible(const acm_dfa *d) { return d && d->sparse_ok ? 1 : 0; }
extern "C" int acm_scan_lds_resident(const acm_dfa *d) { return d && d->lds_ok && d->use_halo ? 1 : 0; }
extern "C" int acm_scan_group_capable(const acm_dfa *d)
{
	if (!d || d->use_graphs || d->max_group <= 1)
		return 0;
	const bool sparse = d->sparse_ok && d->scan_mode != ACM_SCAN_MODE_CHAIN;
	return (sparse || (d->lds_ok && d->use_halo)) ? 1 : 0;
}

extern "C" int acm_scan_path_taken(const acm_dfa *d, const void *d_workspace, size_t n, void *stream)
{
	if (!d || !d_workspace)
		return acm::fail(ACM_ERR_ARG, "acm_scan_path_taken: bad arguments");
	ACM_HIP_TRY(hipSetDevice(d->device));
	uint32_t marker = ACM_SCAN_MODE_CHAIN;   // (an empty text); else written by whichever pipeline produced the planes
	if (n)   // read on the caller's stream: the legacy stream would wait for, or be refused because of, other threads' streams
		ACM_HIP_TRY(hipMemcpyAsync(&marker, (const char *)d_workspace + acm::scan_layout(d, n).misc + 4 * acm::kMiscPath, 4,
		    hipMemcpyDeviceToHost, (hipStream_t)stream));
	ACM_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
	return (int)marker;
}

// The kernels of one scan are short and many; a host that scans with the same
// buffers over and over (a worker with its staging buffers, as the reference's
// workers do) pays more for launching them than the GPU for running them.  So
// the enqueue of a batch that repeats is captured once into a HIP graph and
// replayed with one hipGraphLaunch.
extern "C" int acm_scan_batch_async(const acm_dfa *d, const acm_scan_batch *batch)
{
	if (!batch)
		return acm::fail(ACM_ERR_ARG, "acm_scan_batch_async: null batch");
	const bool sparse = d && pick_sparse(d, batch->n);
	if (!d || !d->use_graphs || d->profile || batch->profile || !batch->stream || batch->wait_before_walk ||
	    batch->record_after_walk || batch->n == 0)
		return enqueue_batch(d, batch, sparse);
	hipStream_t s = (hipStream_t)batch->stream;
	const acm_dfa::GraphKey key = graph_key(d, batch, sparse);
	hipGraphExec_t exec = nullptr;
	bool capture = false;
	{
		std::lock_guard<std::mutex> lock(d->graph_mutex);
		acm_dfa::GraphEntry *e = nullptr;
		for (auto &g : d->graphs)
			if (!memcmp(&g.key, &key, sizeof(key)))
				e = &g;
		if (!e) {   // first sighting: remember it, enqueue the plain way
			if (d->graphs.size() >= acm_dfa::kMaxGraphs) {
				size_t oldest = 0;
				for (size_t i = 1; i < d->graphs.size(); i++)
					if (d->graphs[i].last_use < d->graphs[oldest].last_use)
						oldest = i;
				// its last launch may still be running: an exec is only ever destroyed by
				// acm_dfa_release; an evicted one is parked until then
				if (d->graphs[oldest].exec)
					d->parked_graphs.push_back(d->graphs[oldest].exec);
				d->graphs.erase(d->graphs.begin() + (long)oldest);
			}
			acm_dfa::GraphEntry fresh;
			fresh.key = key;
			fresh.exec = nullptr;
			fresh.last_use = ++d->graph_tick;
			d->graphs.push_back(fresh);
		} else {
			e->last_use = ++d->graph_tick;
			exec = (hipGraphExec_t)e->exec;
			capture = !exec;
		}
	}
	if (exec) {
		ACM_HIP_TRY(hipSetDevice(d->device));
		ACM_HIP_TRY(hipGraphLaunch(exec, s));
		d->graphs_launched.fetch_add(1, std::memory_order_relaxed);
		return ACM_OK;
	}
	if (!capture)
		return enqueue_batch(d, batch, sparse);
	// second sighting: capture.  Argument errors surface here exactly as in the plain path.
	ACM_HIP_TRY(hipSetDevice(d->device));
	if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
		(void)hipGetLastError();
		d->use_graphs = false;   // e.g. the caller is capturing this stream itself
		return enqueue_batch(d, batch, sparse);
	}
	const int rc = enqueue_batch(d, batch, sparse);
	hipGraph_t graph = nullptr;
	const hipError_t end = hipStreamEndCapture(s, &graph);
	if (rc != ACM_OK || end != hipSuccess || !graph) {
		if (graph)
			hipGraphDestroy(graph);
		(void)hipGetLastError();
		d->use_graphs = false;
		return rc != ACM_OK ? rc : enqueue_batch(d, batch, sparse);
	}
	const hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
	hipGraphDestroy(graph);
	if (inst != hipSuccess || !exec) {
		(void)hipGetLastError();
		d->use_graphs = false;
		return enqueue_batch(d, batch, sparse);
	}
	d->graphs_captured.fetch_add(1, std::memory_order_relaxed);
	{
		std::lock_guard<std::mutex> lock(d->graph_mutex);
		bool stored = false;
		for (auto &g : d->graphs)
			if (!memcmp(&g.key, &key, sizeof(key)) && !g.exec) {
				g.exec = (void *)exec;
				stored = true;
			}
		if (!stored)   // evicted, or another thread was quicker
			d->parked_graphs.push_back((void *)exec);   // cannot be destroyed while in flight (nor leaked if the launch fails)
	}
	ACM_HIP_TRY(hipGraphLaunch(exec, s));
	d->graphs_launched.fetch_add(1, std::memory_order_relaxed);
	return ACM_OK;
}

extern "C" int acm_scan_async(const acm_dfa *d, const void *d_text, size_t n, long init_state,
    void *d_workspace, size_t workspace_bytes, int32_t *d_pat_plane, int32_t *d_off_plane,
    size_t plane_capacity, void *stream)
{
	return acm_scan_shard_async(d, d_text, n, 0, 0, init_state, d_workspace, workspace_bytes,
	    d_pat_plane, d_off_plane, plane_capacity, stream);
}

extern "C" int acm_scan_shard_async(const acm_dfa *d, const void *d_text, size_t n, size_t halo,
    long offset_shift, long init_state, void *d_workspace, size_t workspace_bytes,
    int32_t *d_pat_plane, int32_t *d_off_plane, size_t plane_capacity, void *stream)
{
	const acm_scan_batch b = { d_text, n, halo, offset_shift, init_state, d_workspace, workspace_bytes, d_pat_plane,
		d_off_plane, plane_capacity, stream };   // (no events, HEAD records, not timed, no d_init_plane)
	return acm_scan_batch_async(d, &b);
}

extern "C" int acm_scan_batches_async(const acm_dfa *d, const acm_scan_batch *batches, size_t count)
{
	if (!batches && count)
		return acm::fail(ACM_ERR_ARG, "acm_scan_batches_async: null batches");
	if (!d || d->use_graphs || d->max_group <= 1) {
		for (size_t i = 0; i < count; i++) {
			const int rc = acm_scan_batch_async(d, &batches[i]);
			if (rc != ACM_OK)
				return rc;
		}
		return ACM_OK;
	}
	const uint32_t cap = std::min<uint32_t>((uint32_t)d->max_group, max_group_limit());
	const acm_scan_batch *group[32];
	uint32_t m = 0;
	bool group_sparse = true;   // the pipeline of the group being collected
	auto flush = [&]() -> int {
		const uint32_t members = m;
		m = 0;
		if (members > 1)
			return enqueue_group(d, group, members, group_sparse);
		return members ? enqueue_batch(d, group[0], group_sparse) : ACM_OK;
	};
	for (size_t i = 0; i < count; i++) {
		const acm_scan_batch &b = batches[i];
		const bool sparse = pick_sparse(d, b.n);   // (counts the batch: once per batch)
		if ((sparse || lds_path(d, sparse, b.n)) && groupable(d, b)) {
			if (m && (m >= cap || sparse != group_sparse || !joins(group, m, b))) {
				const int rc = flush();
				if (rc != ACM_OK)
					return rc;
			}
			group_sparse = sparse;
			group[m++] = &b;
			continue;
		}
		int rc = flush();
		if (rc == ACM_OK)
			rc = enqueue_batch(d, &b, sparse);
		if (rc != ACM_OK)
			return rc;
	}
	return flush();
}

extern "C" int acm_scan_graph_stats(const acm_dfa *d, uint64_t *captured, uint64_t *launched)
{
	if (!d)
		return acm::fail(ACM_ERR_ARG, "acm_scan_graph_stats: null dfa");
	if (captured)
		*captured = d->graphs_captured.load(std::memory_order_relaxed);
	if (launched)
		*launched = d->graphs_launched.load(std::memory_order_relaxed);
	return ACM_OK;
}

extern "C" int acm_scan_set_max_group(acm_dfa *d, int batches)
{
	if (!d)
		return 1;
	if (batches >= 1)
		d->max_group = std::min<int>(batches, (int)max_group_limit());
	return d->max_group;
}

extern "C" int acm_scan_set_graphs(acm_dfa *d, int enable)
{
	if (!d)
		return 0;
	if (enable >= 0)
		d->use_graphs = enable != 0;
	return d->use_graphs ? 1 : 0;
}

extern "C" int acm_scan_profile_enable(acm_dfa *d, int enable)
{
	if (!d)
		return acm::fail(ACM_ERR_ARG, "acm_scan_profile_enable: null dfa");
	d->profile = enable != 0;
	return ACM_OK;
}

extern "C" int acm_scan_profile_read(acm_dfa *d, double *first_ms, double *second_ms, double *pipeline_ms,
    int *launches)
{
	if (!d)
		return acm::fail(ACM_ERR_ARG, "acm_scan_profile_read: null dfa");
	double first = 0, second = 0, pipe = 0;
	int n = 0;
	std::lock_guard<std::mutex> lock(d->profile_mutex);
	for (size_t i = 0; i + 3 < d->profile_events.size(); i += 4) {
		hipEvent_t e[4];
		for (int k = 0; k < 4; k++)
			e[k] = (hipEvent_t)d->profile_events[i + k];
		float a = 0, b = 0, c = 0;
		ACM_HIP_TRY(hipEventSynchronize(e[3]));
		ACM_HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
		ACM_HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
		ACM_HIP_TRY(hipEventElapsedTime(&c, e[0], e[3]));
		first += a;
		second += b;
		pipe += c;
		n++;
		for (int k = 0; k < 4; k++)
			d->profile_pool.push_back((void *)e[k]);
	}
	d->profile_events.clear();
	if (first_ms) *first_ms = first;
	if (second_ms) *second_ms = second;
	if (pipeline_ms) *pipeline_ms = pipe;
	if (launches) *launches = n;
	return ACM_OK;
}
