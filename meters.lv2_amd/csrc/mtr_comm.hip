// mtr_comm.hip — the one collective of a multi-GPU job: RCCL behind the C ABI (the mtr_comm_* of include/mtr_engine.h), and the
// grouped pair of all-reduces mtr_engine_reduce ends with.  The only TU of the library that sees RCCL's header.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <thread>

#include "mtr_internal.h"
#include "mtr_host.h"

struct mtr_comm {
	ncclComm_t comm = nullptr;
	int rank = 0, world = 1, device = 0;
	bool nonblocking = false;          // built by mtr_comm_init_timeout: every call on it is polled to a deadline
	uint32_t timeout_ms = 0;
	hipStream_t probe_stream = nullptr;
	int32_t* probe_buf = nullptr;
};

static int nccl_fail (const char* what, ncclResult_t r)
{
	char buf[256];
	snprintf (buf, sizeof (buf), "%s: %s", what, ncclGetErrorString (r));
	return fail (MTR_ERR_HIP, buf);
}

static double ms_since (std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli> (std::chrono::steady_clock::now () - t0).count ();
}

// the communicator is beyond repair (a deadline passed, an asynchronous error): abort it; only mtr_comm_destroy may follow
static void comm_abort (mtr_comm* c)
{
	if (c->comm) (void) ncclCommAbort (c->comm);
	c->comm = nullptr;
}

// A call on a non-blocking communicator returned ncclInProgress: poll its state until RCCL has taken the call in, it has
// failed, or the deadline passes (then the communicator is aborted).  `t0` = when the call was made.
static int comm_wait (mtr_comm* c, uint32_t timeout_ms, std::chrono::steady_clock::time_point t0, const char* what)
{
	for (;;) {
		ncclResult_t state = ncclSuccess;
		const ncclResult_t r = ncclCommGetAsyncError (c->comm, &state);
		if (r != ncclSuccess) { comm_abort (c); return nccl_fail (what, r); }
		if (state == ncclSuccess) return MTR_OK;
		if (state != ncclInProgress) { comm_abort (c); return nccl_fail (what, state); }
		if (timeout_ms && ms_since (t0) >= (double) timeout_ms) {
			comm_abort (c);
			char buf[160];
			snprintf (buf, sizeof (buf), "%s: no answer from RCCL within %u ms (communicator aborted)", what, timeout_ms);
			return fail (MTR_ERR_TIMEOUT, buf);
		}
		std::this_thread::sleep_for (std::chrono::microseconds (200));
	}
}

int comm_check (const mtr_comm* c, int device)
{
	if (!c->comm) return fail (MTR_ERR_ARG, "mtr_engine_reduce: the communicator has been aborted");
	if (c->device != device) return fail (MTR_ERR_ARG, "mtr_engine_reduce: engine and communicator sit on different devices");
	return MTR_OK;
}

int comm_all_reduce (mtr_comm* c, int32_t* d_hist, float* d_max, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	// one group: RCCL launches the sum and the max together (6 KB + 16 B: both are pure latency on xGMI)
	const auto t0 = std::chrono::steady_clock::now ();
	ncclResult_t r = ncclGroupStart ();
	if (r != ncclSuccess) return nccl_fail ("ncclGroupStart", r);
	const ncclResult_t r1 = ncclAllReduce (d_hist, d_hist, 2 * MTR_HIST_LEN, ncclInt32, ncclSum, c->comm, st);
	const ncclResult_t r2 = ncclAllReduce (d_max, d_max, 4, ncclFloat32, ncclMax, c->comm, st);
	r = ncclGroupEnd ();
	if (r1 != ncclSuccess && r1 != ncclInProgress) return nccl_fail ("ncclAllReduce (histograms)", r1);
	if (r2 != ncclSuccess && r2 != ncclInProgress) return nccl_fail ("ncclAllReduce (peaks)", r2);
	if (r == ncclInProgress && c->nonblocking) { const int rc = comm_wait (c, c->timeout_ms, t0, "ncclGroupEnd (mtr_engine_reduce)"); if (rc) return rc; }
	else if (r != ncclSuccess) return nccl_fail ("ncclGroupEnd", r);
	return MTR_OK;
}

extern "C" {

int mtr_rccl_version (void)
{
	int v = 0;
	const ncclResult_t r = ncclGetVersion (&v);
	if (r != ncclSuccess) return nccl_fail ("ncclGetVersion", r);
	return v;
}

int mtr_comm_unique_id (void* id128)
{
	static_assert (sizeof (ncclUniqueId) == MTR_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
	if (!id128) return fail (MTR_ERR_ARG, "mtr_comm_unique_id: null argument");
	ncclUniqueId id;
	const ncclResult_t r = ncclGetUniqueId (&id);
	if (r != ncclSuccess) return nccl_fail ("ncclGetUniqueId", r);
	memcpy (id128, &id, sizeof (id));
	return MTR_OK;
}

int mtr_comm_init_timeout (mtr_comm** out, int rank, int world, const void* id128, int device, uint32_t timeout_ms, float* init_ms)
{
	if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return fail (MTR_ERR_ARG, "mtr_comm_init: bad argument");
	*out = nullptr;
	if (init_ms) *init_ms = 0.f;
	int ndev = 0;
	if (hipGetDeviceCount (&ndev) != hipSuccess || ndev <= 0) return fail (MTR_ERR_NODEVICE, "no HIP device");
	if (device < 0 || device >= ndev) return fail (MTR_ERR_ARG, "device ordinal out of range");
	HIPCHK (hipSetDevice (device));
	mtr_comm* c = new (std::nothrow) mtr_comm ();
	if (!c) return fail (MTR_ERR_NOMEM, "new mtr_comm");
	c->rank = rank; c->world = world; c->device = device;
	c->nonblocking = timeout_ms != 0; c->timeout_ms = timeout_ms;
	ncclUniqueId id;
	memcpy (&id, id128, sizeof (id));
	const auto t0 = std::chrono::steady_clock::now ();
	int rc = MTR_OK;
	if (!c->nonblocking) {
		const ncclResult_t r = ncclCommInitRank (&c->comm, world, id, rank);
		if (r != ncclSuccess) { c->comm = nullptr; rc = nccl_fail ("ncclCommInitRank", r); }
	} else {
		// the header may be newer than the RCCL this process runs (torch ships its own): never claim a newer version than the library's
		ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
		int lib_version = 0;
		if (ncclGetVersion (&lib_version) == ncclSuccess && lib_version > 0 && (unsigned) lib_version < cfg.version) cfg.version = (unsigned) lib_version;
		cfg.blocking = 0;
		const ncclResult_t r = ncclCommInitRankConfig (&c->comm, world, id, rank, &cfg);
		if (r != ncclSuccess && r != ncclInProgress) { c->comm = nullptr; rc = nccl_fail ("ncclCommInitRankConfig", r); }
		else if (!c->comm) rc = fail (MTR_ERR_HIP, "ncclCommInitRankConfig returned no communicator");
		else rc = comm_wait (c, timeout_ms, t0, "ncclCommInitRankConfig");
	}
	if (rc == MTR_OK) {
		if (hipStreamCreateWithFlags (&c->probe_stream, hipStreamNonBlocking) != hipSuccess || hipMalloc ((void**) &c->probe_buf, sizeof (int32_t)) != hipSuccess)
			rc = fail (MTR_ERR_HIP, "mtr_comm_init: probe stream / buffer");
	}
	if (init_ms) *init_ms = (float) ms_since (t0);
	if (rc != MTR_OK) { mtr_comm_destroy (c); return rc; }
	*out = c;
	return MTR_OK;
}

int mtr_comm_init (mtr_comm** out, int rank, int world, const void* id128, int device)
{
	return mtr_comm_init_timeout (out, rank, world, id128, device, 0, nullptr);
}

int mtr_comm_set_timeout (mtr_comm* c, uint32_t timeout_ms)
{
	if (!c) return fail (MTR_ERR_ARG, "mtr_comm_set_timeout: null communicator");
	if (!c->nonblocking && timeout_ms) return fail (MTR_ERR_ARG, "mtr_comm_set_timeout: a communicator built by mtr_comm_init blocks; use mtr_comm_init_timeout");
	c->timeout_ms = timeout_ms;
	return MTR_OK;
}

void mtr_comm_destroy (mtr_comm* c)
{
	if (!c) return;
	(void) hipSetDevice (c->device);
	if (c->comm && !c->nonblocking) (void) ncclCommDestroy (c->comm);
	else if (c->comm) {
		// a healthy communicator with a deadline: finalise (collectives still queued complete), polled to the deadline, then
		// destroy; abort only if that does not happen in time (abort kills a reduce that is still queued)
		const auto t0 = std::chrono::steady_clock::now ();
		const uint32_t limit = c->timeout_ms ? c->timeout_ms : 10000u;
		ncclResult_t r = ncclCommFinalize (c->comm);
		bool ok = r == ncclSuccess || r == ncclInProgress;
		while (ok) {
			ncclResult_t state = ncclSuccess;
			if (ncclCommGetAsyncError (c->comm, &state) != ncclSuccess || (state != ncclSuccess && state != ncclInProgress)) { ok = false; break; }
			if (state == ncclSuccess) break;
			if (ms_since (t0) >= (double) limit) { ok = false; break; }
			std::this_thread::sleep_for (std::chrono::microseconds (200));
		}
		if (ok) (void) ncclCommDestroy (c->comm); else (void) ncclCommAbort (c->comm);
	}
	c->comm = nullptr;
	if (c->probe_buf) (void) hipFree (c->probe_buf);
	if (c->probe_stream) (void) hipStreamDestroy (c->probe_stream);
	delete c;
}

int mtr_comm_probe (mtr_comm* c, uint32_t timeout_ms, float* ms)
{
	if (ms) *ms = 0.f;
	if (!c) return fail (MTR_ERR_ARG, "mtr_comm_probe: null communicator");
	if (!c->comm) return fail (MTR_ERR_ARG, "mtr_comm_probe: the communicator has been aborted");
	// (every failure from here on leaves the communicator aborted, as the header says)
#define PROBECHK(call) do { hipError_t he_ = (call); if (he_ != hipSuccess) { comm_abort (c); return fail (MTR_ERR_HIP, #call, he_); } } while (0)
	PROBECHK (hipSetDevice (c->device));
	const int32_t one = 1;
	PROBECHK (hipMemcpyAsync (c->probe_buf, &one, sizeof (one), hipMemcpyHostToDevice, c->probe_stream));
	PROBECHK (hipStreamSynchronize (c->probe_stream));
	const auto t0 = std::chrono::steady_clock::now ();
	const ncclResult_t r = ncclAllReduce (c->probe_buf, c->probe_buf, 1, ncclInt32, ncclSum, c->comm, c->probe_stream);
	if (r != ncclSuccess && r != ncclInProgress) { comm_abort (c); return nccl_fail ("ncclAllReduce (probe)", r); }
	if (c->nonblocking) { const int rc = comm_wait (c, timeout_ms, t0, "ncclAllReduce (probe)"); if (rc) return rc; }
	// the collective itself: poll the stream, and the communicator for an asynchronous error (a peer that died)
	for (;;) {
		const hipError_t q = hipStreamQuery (c->probe_stream);
		if (q == hipSuccess) break;
		if (q != hipErrorNotReady) { comm_abort (c); return fail (MTR_ERR_HIP, "hipStreamQuery (probe)", q); }
		ncclResult_t state = ncclSuccess;
		if (ncclCommGetAsyncError (c->comm, &state) == ncclSuccess && state != ncclSuccess && state != ncclInProgress) { comm_abort (c); return nccl_fail ("ncclAllReduce (probe)", state); }
		if (timeout_ms && ms_since (t0) >= (double) timeout_ms) {
			comm_abort (c);
			char buf[160];
			snprintf (buf, sizeof (buf), "mtr_comm_probe: the first all-reduce did not finish within %u ms (communicator aborted)", timeout_ms);
			return fail (MTR_ERR_TIMEOUT, buf);
		}
		std::this_thread::sleep_for (std::chrono::microseconds (100));
	}
	if (ms) *ms = (float) ms_since (t0);
	int32_t got = 0;
	PROBECHK (hipMemcpy (&got, c->probe_buf, sizeof (got), hipMemcpyDeviceToHost));
#undef PROBECHK
	if (got != c->world) {
		char buf[160];
		snprintf (buf, sizeof (buf), "mtr_comm_probe: all-reduce of ones over %d ranks gave %d", c->world, (int) got);
		comm_abort (c);
		return fail (MTR_ERR_HIP, buf);
	}
	return MTR_OK;
}

int mtr_comm_nranks (mtr_comm* c)
{
	if (!c) return fail (MTR_ERR_ARG, "mtr_comm_nranks: null communicator");
	if (!c->comm) return fail (MTR_ERR_ARG, "mtr_comm_nranks: the communicator has been aborted");
	int n = 0;
	const ncclResult_t r = ncclCommCount (c->comm, &n);
	if (r != ncclSuccess) return nccl_fail ("ncclCommCount", r);
	return n;
}

int mtr_comm_device (mtr_comm* c)
{
	if (!c) return fail (MTR_ERR_ARG, "mtr_comm_device: null communicator");
	if (!c->comm) return fail (MTR_ERR_ARG, "mtr_comm_device: the communicator has been aborted");
	int d = -1;
	const ncclResult_t r = ncclCommCuDevice (c->comm, &d);
	if (r != ncclSuccess) return nccl_fail ("ncclCommCuDevice", r);
	return d;
}
} // extern "C"
