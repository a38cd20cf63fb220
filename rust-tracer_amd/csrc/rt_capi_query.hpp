// rt_capi_query.hpp -- part of rt_capi.hip: what the query entries of rt_capi_entry.hpp share -- how a call reaches the caller's host
// buffers (HostStaging) and the skeletons of a single-pass query and of a two-pass list query, each for host and for device memory.  A
// new query brings its table of buffers and its enqueue calls; nothing here knows which entry runs it.  What the layer below shares --
// the precision and flavour switches, the alignment check, the domain predicates -- stands at the head of rt_capi_launch.hpp's query
// part; DESIGN.md 4.6 ("Where the host side of a query lives") lists what a new query has to bring to each layer.
// (included by rt_capi.hip where its text used to stand: nothing here is a header of its own)

struct HostDest { bool pinned = false; uint8_t *dev_alias = nullptr; bool bad = false; size_t room = 0; };

// Host ranges this library pinned itself (rt_host_alloc / rt_host_register), base -> {bytes, device alias}.  Only these are
// written by the render kernel directly.  Asking the runtime instead (hipPointerGetAttributes) is not safe: it also reports
// ranges it locked on its own for an earlier pageable copy, and such a record can outlive the caller's buffer -- a kernel
// store to it is a GPU memory fault (seen as an intermittent fault on freshly allocated numpy buffers).
struct PinnedRange { size_t bytes; uint8_t *alias; };
std::mutex g_pinned_mu;
std::map<uintptr_t, PinnedRange> g_pinned;

HostDest classify_host_pointer(const void *p)
{
    HostDest d;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        auto it = g_pinned.upper_bound(a);
        if (it != g_pinned.begin()) {
            --it;
            if (a - it->first < it->second.bytes) {
                d.pinned = true;
                d.dev_alias = it->second.alias ? it->second.alias + (a - it->first) : nullptr;
                d.room = it->second.bytes - (a - it->first);
                return d;
            }
        }
    }
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return d; }      // plain pageable memory
    if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray) d.bad = true;            // a device pointer is a caller error here
    return d;
}

// From a host call's first copy on, work of it may be queued on its context's stream: an error return first waits for it, so that the
// context is not handed to the next caller with work in flight.  A failed step of our own also leaves the runtime's sticky error cleared.
rt_status drain(Context *c, rt_status st)
{
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    return st;
}

rt_status hip_drain(Context *c, hipError_t e, const char *expr, int line, const char *file = __builtin_FILE())
{
    if (e == hipSuccess) return RT_OK;
    (void)hipStreamSynchronize(c->stream);
    return hip_fail(e, expr, line, file);
}

#define HIP_TRY_DRAIN(c, expr)                                                                                            \
    do {                                                                                                                  \
        if (const rt_status st__ = hip_drain((c), (expr), #expr, __LINE__); st__ != RT_OK) return st__;                   \
    } while (0)

// The host buffers of one call.  Every buffer is either the caller's own memory, read and written by the kernels in place (rt_host_alloc /
// rt_host_register), or a device copy in the call's workspace c->d_query (pageable memory, or a pinned range too small for the row: the
// copies go through the runtime's staging).  An entry fills the rows; a NULL row is skipped and resolves to a NULL device pointer.
enum StageDir { kStageIn, kStageOut };

struct HostStaging {
    // unit != 0: an output list of `unit`-byte entries of which only a written prefix is copied back (download_prefix)
    struct Row { const void *host; size_t bytes; StageDir dir; size_t unit = 0; uint8_t *dev = nullptr; size_t off = 0; bool staged = false; };
    Row *row;
    int n;
    size_t need = 0;

    template <int N> explicit HostStaging(Row (&rows)[N]) : row(rows), n(N) {}

    // Where every row lives; no device work.  Device memory is refused, also as `refuse_only`: a pointer the CPU alone writes.
    // in_place == false: every row is staged, whatever memory it is.
    rt_status plan(const char *what, const void *refuse_only = nullptr, bool in_place = true)
    {
        need = 0;
        for (int i = 0; i < n; ++i) {
            Row &x = row[i];
            if (!x.host) continue;
            const HostDest d = classify_host_pointer(x.host);
            if (d.bad) return refuse(what);
            if (in_place && d.pinned && d.dev_alias && d.room >= x.bytes) { x.dev = d.dev_alias; continue; }
            x.staged = true;
            x.off = need;
            need += (x.bytes + 255) & ~(size_t)255;
        }
        if (refuse_only && classify_host_pointer(refuse_only).bad) return refuse(what);
        return RT_OK;
    }

    // Room in the context's workspace for the staged rows, and their device pointers.
    rt_status bind(Context *c)
    {
        if (need > c->query_cap) {
            if (c->d_query) HIP_TRY(hipFree(c->d_query));
            c->d_query = nullptr; c->query_cap = 0;
            HIP_TRY(hipMalloc(&c->d_query, need));
            c->query_cap = need;
        }
        for (int i = 0; i < n; ++i)
            if (row[i].staged) row[i].dev = static_cast<uint8_t *>(c->d_query) + row[i].off;
        return RT_OK;
    }

    template <typename T = void> T *dev(int i) const { return reinterpret_cast<T *>(row[i].dev); }

    rt_status upload(Context *c) const
    {
        for (int i = 0; i < n; ++i)
            if (row[i].staged && row[i].dir == kStageIn)
                HIP_TRY_DRAIN(c, hipMemcpyAsync(row[i].dev, row[i].host, row[i].bytes, hipMemcpyHostToDevice, c->stream));
        return RT_OK;
    }

    // the whole of every staged output that is no list
    rt_status download(Context *c) const
    {
        for (int i = 0; i < n; ++i)
            if (row[i].staged && row[i].dir == kStageOut && row[i].unit == 0)
                HIP_TRY_DRAIN(c, hipMemcpyAsync(const_cast<void *>(row[i].host), row[i].dev, row[i].bytes, hipMemcpyDeviceToHost, c->stream));
        return RT_OK;
    }

    // the first `count` entries of list row i (only what was written: the caller's bytes behind it stay)
    rt_status download_prefix(Context *c, int i, size_t count) const
    {
        if (row[i].staged)
            HIP_TRY_DRAIN(c, hipMemcpyAsync(const_cast<void *>(row[i].host), row[i].dev, row[i].unit * count, hipMemcpyDeviceToHost, c->stream));
        return RT_OK;
    }

private:
    static rt_status refuse(const char *what)
    {
        snprintf(g_err, sizeof g_err, "%s: a buffer is device memory; use %s_device", what, what);
        return RT_ERR_INVALID_ARGUMENT;
    }
};

// A call that counts: its counters cleared and the start of its interval on `stream`.
rt_status stats_begin(Context *c, hipStream_t stream)
{
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(rt::Counters) * rt::kCounterStripes, stream));
    HIP_TRY(hipEventRecord(c->ev0, stream));
    return RT_OK;
}

rt_status no_pre_step(Context *) { return RT_OK; }

// A single-pass query over host buffers, `hs` planned: the staged inputs up, the entry's kernels, the staged outputs back, all on the
// leased context's stream, which is drained before the call returns.
//   pre(c)                                       what runs before the counted interval (the ordered entries' own sort), or no_pre_step
//   enqueue(nodes, n_nodes, counters, stream)    the entry's kernels on hs's device pointers; counters: NULL unless stats is given
//   read_stats                                   read_query_stats or read_trace_stats
template <typename Pre, typename Enqueue>
rt_status host_query(rt_scene *s, HostStaging &hs, rt_stats *stats, rt_status (*read_stats)(Context *, hipStream_t, rt_stats *), Pre &&pre, Enqueue &&enqueue)
{
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    rt_status st = RT_OK;
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    if ((st = query_stream(s, c->stream, &nodes, &n_nodes)) != RT_OK) return st;
    if ((st = hs.bind(c)) != RT_OK) return st;
    if ((st = hs.upload(c)) != RT_OK) return st;
    if ((st = pre(c)) != RT_OK) return drain(c, st);
    if (stats && (st = stats_begin(c, c->stream)) != RT_OK) return drain(c, st);
    if ((st = enqueue(nodes, n_nodes, stats ? c->d_counters : nullptr, c->stream)) != RT_OK) return drain(c, st);
    if (stats) HIP_TRY_DRAIN(c, hipEventRecord(c->ev1, c->stream));
    if ((st = hs.download(c)) != RT_OK) return st;
    if (stats) return read_stats(c, c->stream, stats);                // synchronises the stream
    HIP_TRY_DRAIN(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

// The same query over device memory on the caller's stream.  Without stats it acquires no context and returns without waiting.
template <typename Enqueue>
rt_status device_query(rt_scene *s, rt_stats *stats, hipStream_t stream, Enqueue &&enqueue)
{
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    if (!stats) return enqueue(nodes, n_nodes, nullptr, stream);
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    if ((st = stats_begin(c, stream)) != RT_OK) return st;
    st = enqueue(nodes, n_nodes, c->d_counters, stream);
    (void)hipEventRecord(c->ev1, stream);
    if (st != RT_OK) { (void)hipGetLastError(); lease.inflight = true; return st; }      // (the context goes back behind what is enqueued)
    return read_query_stats(c, stream, stats);
}

// A two-pass list query over host buffers, `hs` planned: count, read the total, fill, copy back what was written.  The two passes share
// the scene's workspace `ws` and this call reads the total between them: host calls on one workspace take turns (context lease first,
// ws.mu second).  fill: the caller gave a list and a capacity above 0.
//   begin(nodes, n_nodes, stream)                     the entry's *_begin: the workspace, and this call's place behind the one before it
//   count(nodes, n_nodes, counters, stream)           the first pass and the scan, the total into ws.d_total
//   fill_lists(nodes, n_nodes, stream)                the second pass into hs's list rows
template <typename Begin, typename Count, typename Fill>
rt_status host_list_query(rt_scene *s, ListSpace &ws, HostStaging &hs, uint32_t capacity, bool fill, uint64_t *total_out, rt_stats *stats, Begin &&begin,
                          Count &&count, Fill &&fill_lists)
{
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    rt_status st = RT_OK;
    Context *c = nullptr;
    if ((st = acquire(s, &c)) != RT_OK) return st;
    Lease lease{ s, c };
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    if ((st = query_stream(s, c->stream, &nodes, &n_nodes)) != RT_OK) return st;
    if ((st = hs.bind(c)) != RT_OK) return st;
    std::lock_guard<std::mutex> lk(ws.mu);
    if ((st = begin(nodes, n_nodes, c->stream)) != RT_OK) return st;
    if ((st = hs.upload(c)) != RT_OK) return st;
    if (stats && (st = stats_begin(c, c->stream)) != RT_OK) return drain(c, st);
    // the scan writes the total into the workspace's pinned word: an asynchronous copy into this frame would have the runtime lock a page
    // of the caller's stack, and keep its record of it when the thread and its stack are gone
    if ((st = count(nodes, n_nodes, stats ? c->d_counters : nullptr, c->stream)) != RT_OK) return drain(c, st);
    if ((st = hs.download(c)) != RT_OK) return st;                    // (the offsets)
    HIP_TRY_DRAIN(c, hipStreamSynchronize(c->stream));
    const uint64_t total = *static_cast<volatile uint64_t *>(ws.h_total);
    *total_out = total;
    const size_t written = (size_t)std::min<uint64_t>(total, capacity);
    if (fill && written) {
        if ((st = fill_lists(nodes, n_nodes, c->stream)) != RT_OK) return drain(c, st);
        for (int i = 0; i < hs.n; ++i)
            if (hs.row[i].unit && (st = hs.download_prefix(c, i, written)) != RT_OK) return st;
    }
    if (stats) {
        HIP_TRY_DRAIN(c, hipEventRecord(c->ev1, c->stream));
        return read_query_stats(c, c->stream, stats);                // synchronises the stream
    }
    HIP_TRY_DRAIN(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

// The same query over device memory on the caller's stream: both passes enqueued, nothing read.  Without stats it acquires no context and
// returns without waiting.  fill: as above; the callables as above, count writing the total where the caller wants it.
template <typename Begin, typename Count, typename Fill>
rt_status device_list_query(rt_scene *s, ListSpace &ws, bool fill, rt_stats *stats, hipStream_t stream, Begin &&begin, Count &&count, Fill &&fill_lists)
{
    const ReadLock rl(s);
    HIP_TRY(hipSetDevice(s->device));
    const void *nodes = nullptr;
    uint32_t n_nodes = 0;
    rt_status st = query_stream(s, stream, &nodes, &n_nodes);
    if (st != RT_OK) return st;
    Context *c = nullptr;
    Lease lease{ s, nullptr };
    if (stats) {
        if ((st = acquire(s, &c)) != RT_OK) return st;
        lease.c = c;
    }
    {
        std::lock_guard<std::mutex> lk(ws.mu);
        if ((st = begin(nodes, n_nodes, stream)) != RT_OK) return st;
        if (stats && (st = stats_begin(c, stream)) != RT_OK) return st;
        st = count(nodes, n_nodes, stats ? c->d_counters : nullptr, stream);
        if (st == RT_OK && fill) st = fill_lists(nodes, n_nodes, stream);
        // whatever was enqueued uses the workspace: the next call goes behind it
        if (hipEventRecord(ws.ev, stream) == hipSuccess) ws.recorded = true;
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); }
    }
    if (!stats) return st;
    (void)hipEventRecord(c->ev1, stream);
    if (st != RT_OK) { (void)hipGetLastError(); lease.inflight = true; return st; }      // (the context goes back behind what is enqueued)
    return read_query_stats(c, stream, stats);
}
