// stream_capi.inc -- landing_stream_*: consecutive batches through one context with the GPU kept busy across batch boundaries (VERDICT r5 item 5).
//
// One launch of landing_ipm_kernel ends with its slowest member: a batch of 1024 on the 512 resident slots takes 53 ms while the slots are busy for
// 40 ms on average (DESIGN.md 4.2) -- in the last quarter of a launch most CUs idle behind a handful of members that need 2-4 x the mean iteration
// count.  A caller that streams batches (the data-generation loop of generate_data/generate_training_data_automated.m:38) gets that quarter back when
// the next batch's workgroups fill the slots the previous batch frees: two launches in flight on two HIP streams, each with its own workspace.  Rounds 3-5
// measured it from the outside (two contexts, two streams, two host threads: bench.py `two_batches_in_flight`, 25.0 k against 19.2 k NLPs/s); here the library
// does it behind one call pattern -- submit, submit, ..., wait -- on the caller's one context and one thread.  Lane 0 is the context itself, lanes 1.. are
// child contexts with the same formulation (their own solver workspace: 1.3 MB per member at N = 40), every lane has a non-blocking stream of its own;
// submission i goes to lane i mod lanes, ordered behind the caller's stream (the inputs are ready there) by an event.  Members are independent and a
// lane runs the very launch landing_solve_batch would: results are bit-identical to one call at a time (tests/test_gpu_dataset.py).
struct landing_stream {
  landing_ctx* owner = nullptr;
  std::vector<landing_ctx*> lane;        // lane[0] == owner (not owned)
  std::vector<hipStream_t> st;
  std::vector<hipEvent_t> done;
  std::vector<long long> ticket_of;      // last ticket submitted to a lane (-1: none)
  hipEvent_t in_ready = nullptr;
  long long n_sub = 0;
};

extern "C" {

landing_stream* landing_stream_create(landing_ctx* ctx, int lanes) {
  if (!ctx) { fail(LANDING_E_ARG, "landing_stream_create: bad argument"); return nullptr; }
  if (lanes == 0) lanes = 2;
  if (lanes < 1 || lanes > 8) { fail(LANDING_E_ARG, "landing_stream_create: 1..8 lanes"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { fail(LANDING_E_HIP, "hipSetDevice failed"); return nullptr; }
  landing_stream* s = new landing_stream();
  s->owner = ctx;
  bool ok = hipEventCreateWithFlags(&s->in_ready, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; i < lanes && ok; ++i) {
    landing_ctx* c = ctx;
    if (i > 0) {
      c = landing_create(ctx->L.N, ctx->device, nullptr);
      if (!c) { ok = false; break; }
      c->L = ctx->L;      // same formulation (constraint literals, running cost, parameter layout)
    }
    s->lane.push_back(c);
    hipStream_t q = nullptr; hipEvent_t e = nullptr;
    ok = ok && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess;
    s->st.push_back(q);
    ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    s->done.push_back(e);
    s->ticket_of.push_back(-1);
  }
  if (!ok) { fail(LANDING_E_HIP, "landing_stream_create: lane setup failed"); landing_stream_destroy(s); return nullptr; }
  return s;
}

int landing_stream_lanes(const landing_stream* s) { return s ? (int)s->lane.size() : 0; }

long long landing_stream_submit(landing_stream* s, int B, const double* d_p, const double* d_x0, const landing_solver_opts* opts,
                                double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters, double* d_kkt, void* in_stream) {
  if (!s || B < 0 || (B > 0 && (!d_p || !d_x0 || !d_x))) return fail(LANDING_E_ARG, "landing_stream_submit: bad argument");
  HIP_TRY(hipSetDevice(s->owner->device));
  const int l = (int)(s->n_sub % (long long)s->lane.size());
  HIP_TRY(hipEventRecord(s->in_ready, (hipStream_t)in_stream));      // whatever produced d_p / d_x0 on the caller's stream comes first
  HIP_TRY(hipStreamWaitEvent(s->st[l], s->in_ready, 0));
  landing_ctx* c = s->lane[l];
  const int rc = landing_solve_batch(c, B, d_p, d_x0, opts, d_x, d_f, d_lam_g, d_status, d_iters, d_kkt, (void*)s->st[l]);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->done[l], s->st[l]));
  s->ticket_of[l] = s->n_sub;
  return s->n_sub++;
}

// `stream` != NULL: that stream waits for the submission (no host synchronisation); NULL: the host waits.  A ticket whose lane has been used
// again since is complete once the later submission of that lane is (stream order), so waiting for the lane's last event covers it.
int landing_stream_wait(landing_stream* s, long long ticket, void* stream) {
  if (!s || ticket < 0 || ticket >= s->n_sub) return fail(LANDING_E_ARG, "landing_stream_wait: no such ticket");
  HIP_TRY(hipSetDevice(s->owner->device));
  const int l = (int)(ticket % (long long)s->lane.size());
  if (stream) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, s->done[l], 0));
  else HIP_TRY(hipEventSynchronize(s->done[l]));
  return 0;
}

int landing_stream_sync(landing_stream* s, void* stream) {
  if (!s) return fail(LANDING_E_ARG, "landing_stream_sync: bad argument");
  for (size_t l = 0; l < s->lane.size(); ++l) if (s->ticket_of[l] >= 0) { const int rc = landing_stream_wait(s, s->ticket_of[l], stream); if (rc) return rc; }
  return 0;
}

void landing_stream_destroy(landing_stream* s) {
  if (!s) return;
  if (s->owner) (void)hipSetDevice(s->owner->device);
  for (size_t l = 0; l < s->st.size(); ++l) if (s->st[l]) { (void)hipStreamSynchronize(s->st[l]); }
  for (size_t l = 0; l < s->done.size(); ++l) if (s->done[l]) (void)hipEventDestroy(s->done[l]);
  for (size_t l = 0; l < s->st.size(); ++l) if (s->st[l]) (void)hipStreamDestroy(s->st[l]);
  for (size_t l = 1; l < s->lane.size(); ++l) if (s->lane[l]) landing_destroy(s->lane[l]);
  if (s->in_ready) (void)hipEventDestroy(s->in_ready);
  delete s;
}

// Host arrays, any number of members: the batch is cut into chunks of `chunk` members (0 = 1024) that go through a stream of `lanes` lanes.  Every
// lane slot has device buffers for one chunk and a copy stream of its own: the upload of chunk i + 1 and the download of chunk i - 1 are queued there
// while chunk i solves.  The copies go straight to and from the caller's pageable host arrays (no pinned staging), so they overlap the solves only as
// far as the runtime's own staging of pageable memory lets them.  Same results as landing_solve_batch_host.
int landing_solve_stream_host(landing_ctx* ctx, int B, int chunk, int lanes, const double* p, const double* x0, const landing_solver_opts* opts,
                              double* x, double* f, double* lam_g, int* status, int* iters, double* kkt) {
  if (!ctx || B < 0 || (B > 0 && (!p || !x0 || !x))) return fail(LANDING_E_ARG, "landing_solve_stream_host: bad argument");
  if (B == 0) return 0;
  if (chunk <= 0) chunk = 1024;
  if (lanes <= 0) lanes = 2;
  const Layout& L = ctx->L;
  std::lock_guard<std::mutex> hs_lock(ctx->hs_mu);
  if (ctx->hs_obj && ctx->hs_lanes != lanes) { landing_stream_destroy(ctx->hs_obj); ctx->hs_obj = nullptr; }
  if (!ctx->hs_obj) { ctx->hs_obj = landing_stream_create(ctx, lanes); ctx->hs_lanes = lanes; }
  landing_stream* s = ctx->hs_obj;      // kept by the context: the child contexts of the lanes and their workspaces are built once
  if (!s) return LANDING_E_HIP;
  const int K = (int)s->lane.size();
  struct Slot { DevBuf<double> p, x0, x, f, l, k; DevBuf<int> si; hipStream_t cp = nullptr; };      // si: status | iters
  std::vector<Slot> slot(K);
  int rc = 0;
  auto bail = [&](int code, const char* what) { rc = fail(code, what); };
  for (int i = 0; i < K && !rc; ++i) {
    Slot& q = slot[i]; const size_t c = (size_t)chunk;
    if (q.p.alloc(c * L.np) != hipSuccess || q.x0.alloc(c * L.nx) != hipSuccess || q.x.alloc(c * L.nx) != hipSuccess || q.f.alloc(c) != hipSuccess ||
        q.l.alloc(c * L.ng) != hipSuccess || q.k.alloc(c * 3) != hipSuccess || q.si.alloc(2 * c) != hipSuccess ||
        hipStreamCreateWithFlags(&q.cp, hipStreamNonBlocking) != hipSuccess)
      bail(LANDING_E_HIP, "landing_solve_stream_host: allocation failed");
  }
  const int nchunk = (B + chunk - 1) / chunk;
  std::vector<long long> tk(nchunk, -1);
  auto download = [&](int ci) {      // D2H of chunk ci on its slot's copy stream, ordered behind its solve
    Slot& q = slot[ci % K]; const size_t b0 = (size_t)ci * chunk, nb = std::min<size_t>(chunk, (size_t)B - b0);
    if (landing_stream_wait(s, tk[ci], (void*)q.cp)) { rc = LANDING_E_HIP; return; }
    int* ds = q.si.get(); int* di = ds + chunk;
    hipError_t e = hipMemcpyAsync(x + b0 * L.nx, q.x.get(), nb * L.nx * 8, hipMemcpyDeviceToHost, q.cp);
    if (e == hipSuccess && f) e = hipMemcpyAsync(f + b0, q.f.get(), nb * 8, hipMemcpyDeviceToHost, q.cp);
    if (e == hipSuccess && lam_g) e = hipMemcpyAsync(lam_g + b0 * L.ng, q.l.get(), nb * L.ng * 8, hipMemcpyDeviceToHost, q.cp);
    if (e == hipSuccess && status) e = hipMemcpyAsync(status + b0, ds, nb * sizeof(int), hipMemcpyDeviceToHost, q.cp);
    if (e == hipSuccess && iters) e = hipMemcpyAsync(iters + b0, di, nb * sizeof(int), hipMemcpyDeviceToHost, q.cp);
    if (e == hipSuccess && kkt) e = hipMemcpyAsync(kkt + b0 * 3, q.k.get(), nb * 3 * 8, hipMemcpyDeviceToHost, q.cp);
    if (e != hipSuccess) bail(LANDING_E_HIP, "landing_solve_stream_host: download failed");
  };
  for (int ci = 0; ci < nchunk && !rc; ++ci) {
    Slot& q = slot[ci % K]; const size_t b0 = (size_t)ci * chunk, nb = std::min<size_t>(chunk, (size_t)B - b0);
    if (ci >= K) { download(ci - K); if (rc) break; if (hipStreamSynchronize(q.cp) != hipSuccess) { bail(LANDING_E_HIP, "landing_solve_stream_host: copy failed"); break; } }      // the slot's buffers are free again
    if (hipMemcpyAsync(q.p.get(), p + b0 * L.np, nb * L.np * 8, hipMemcpyHostToDevice, q.cp) != hipSuccess ||
        hipMemcpyAsync(q.x0.get(), x0 + b0 * L.nx, nb * L.nx * 8, hipMemcpyHostToDevice, q.cp) != hipSuccess) { bail(LANDING_E_HIP, "landing_solve_stream_host: upload failed"); break; }
    int* ds = q.si.get(); int* di = ds + chunk;
    const long long t = landing_stream_submit(s, (int)nb, q.p.get(), q.x0.get(), opts, q.x.get(), q.f.get(), q.l.get(), ds, di, q.k.get(), (void*)q.cp);
    if (t < 0) { rc = (int)t; break; }
    tk[ci] = t;
  }
  for (int ci = std::max(0, nchunk - K); ci < nchunk && !rc; ++ci) if (tk[ci] >= 0) download(ci);
  for (int i = 0; i < K; ++i) if (slot[i].cp) { if (hipStreamSynchronize(slot[i].cp) != hipSuccess && !rc) bail(LANDING_E_HIP, "landing_solve_stream_host: kernel failed"); }
  (void)landing_stream_sync(s, nullptr);
  for (int i = 0; i < K; ++i) if (slot[i].cp) (void)hipStreamDestroy(slot[i].cp);
  return rc;
}

}  // extern "C"
