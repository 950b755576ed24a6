/* filter_hip_mini.h -- small inline masters behind filter.h (included by filter_hip.c only).
 *
 * radiod's filter2 (src/radio.c:1503-1513,1572-1594; share/presets.conf:204,223,297): every channel that asks for it
 * owns a private COMPLEX master of N = round2(2*blocksize) points with ONE same-size COMPLEX slave, shift 0, optionally
 * ISB, and drives it inline from its own thread:
 *     write_cfilter(&filter2.in, first filter's output, olen)  ->  execute_filter_output(&filter2.out, 0)
 * A thousand such masters cannot be a thousand engines.  Here a COMPLEX master of N <= 8192 points is a "mini": it owns
 * nothing on the device but a response row in a pool shared by every mini of its geometry (chz_mini_*, include/chz_engine.h).
 *   execute_filter_input   only book-keeps (job number, where the block's N-sample window sits in the mirrored host ring)
 *                          and publishes the job at once -- there is nothing to wait for;
 *   execute_filter_output  queues the window for the pool's next launch.  The channel threads of one radiod block all
 *                          arrive here within microseconds of each other (they were released together), so the first one
 *                          becomes the batch leader and ONE kernel launch (one workgroup per instance) and ONE round trip
 *                          serve everybody who queued up meanwhile.
 * What a pooled instance cannot do -- a slave whose block size differs from its master's, or a REAL-output slave -- turns a
 * master that is still undecided (mini_wanted) into a full engine at that create_filter_output (round 6); on a master that
 * already serves a same-size slave it fails loudly.
 *
 * REAL masters (ka9q_hip_pool_real_masters(1), default off): wfm's composite master (src/wfm.c:70-89), stereod, rdsd, packetd and ctcss
 * keep a small REAL master per channel or session with one to three decimating slaves and run it inline.  With the option on, and an
 * engine library that has chz_rmini_*, a REAL master of even N <= 16384 starts undecided in the same way: host state only, its slaves
 * register as they are created, and at the first execute_filter_output -- the slave list is final then -- the master joins the pool
 * of its geometry (L, M, the list of (olen, type)); see the second half of this file. */
#define CTX_ENGINE 0x454e47
#define CTX_MINI   0x4d494e
#define CTX_SLAVE  0x534c56         /* struct sctx: a slave of an engine master */
#define CTX_MSLAVE 0x4d534c         /* struct msctx: a slave of a mini master */
#define CTX_RSLAVE 0x52534c         /* struct rsctx: a slave of a pooled REAL master */
#define RM_MAX 4                    /* slaves a pooled REAL master carries (chz_rmini_create) */
struct rmshared;

struct mini_req {
  int inst, shift;
  unsigned char isb;
  const float *win;
  float *out;
  int rc;
  bool done;
  struct mini_req *next;
};

struct minipool {
  int L, M, cap, used;
  chz_mini *h;
  pthread_mutex_t lock;
  pthread_cond_t cv;
  struct mini_req *head, *tail;
  bool leader;
  struct minipool *next;
};

struct minictx {                    /* hangs off master->fwd_plan */
  int kind;                         /* CTX_MINI */
  int nslaves;                      /* slaves created on this master and not yet deleted */
  bool decided;                     /* a same-size COMPLEX slave has been created: this master IS a pooled inline master (see mini_wanted) */
  struct filter_in *master;
  const void *job_win[ND];          /* start of the N-sample window of the job in each slot */
  struct rmshared *rs;              /* a REAL master: what it shares with its slaves (and what outlives it when it is deleted first) */
};
struct msctx {                      /* hangs off slave->rev_plan */
  int kind;                         /* CTX_MSLAVE */
  struct minipool *pool;
  int inst;
};

static pthread_mutex_t Mini_registry_lock = PTHREAD_MUTEX_INITIALIZER;
static struct minipool *Mini_pools;

static bool smooth235(int n) { for (int p = 2; p <= 5; p++) while (p != 4 && n % p == 0) n /= p; return n == 1; }
/* A small COMPLEX master MAY be radiod's filter2 -- or the front end of a Funcube dongle (192 kHz: N = 4800) or an Airspy HF+ at its low rates.
   create_filter_input cannot tell, so such a master starts UNDECIDED (host state only): the first same-size COMPLEX create_filter_output makes it a
   pooled inline master (filter2 creates its slave right behind its master, src/radio.c:1583-1585); any other kind of slave, or a first block
   arriving while it has no slave at all (a front end streams before its channels exist), makes it a full engine -- in place: ring, pointers and
   job counter stay (round 6; rounds 2-5 refused every decimating slave of such a front end). */
static bool mini_wanted(int L, int M, enum filtertype in_type) {
  const char *e = XENV("KA9Q_HIP_MINI");
  if (e && e[0] == '0') return false;
  int const N = L + M - 1;
  return in_type == COMPLEX && N >= 8 && N <= 8192 && smooth235(N);
}
static bool is_mini_master(const struct filter_in *m) {
  if (!m) return false;
  const void *const ctx = __atomic_load_n((void *const *)(void *)&m->fwd_plan, __ATOMIC_ACQUIRE);      /* (swapped once, when an undecided master becomes an engine) */
  return ctx && *(const int *)ctx == CTX_MINI;
}

/* a pool of this geometry with a free instance (created on demand) */
static struct minipool *mini_pool_for(int L, int M) {
  pthread_mutex_lock(&Mini_registry_lock);
  struct minipool *p = Mini_pools;
  while (p && !(p->L == L && p->M == M && p->used < p->cap)) p = p->next;
  if (!p) {
    p = calloc(1, sizeof *p);
    if (p) {
      const char *e = XENV("KA9Q_HIP_MINI_POOL");
      const char *dev = getenv("KA9Q_HIP_DEVICE");
      p->L = L; p->M = M; p->cap = e && atoi(e) > 0 ? atoi(e) : 1024;
      if (chz_mini_create(&p->h, L, M, p->cap, dev ? atoi(dev) : 0) != 0) {
        fprintf(stderr, "filter_hip: mini-master pool L=%d M=%d: %s\n", L, M, chz_last_error());
        free(p); p = NULL;
      } else {
        pthread_mutex_init(&p->lock, NULL);
        pthread_cond_init(&p->cv, NULL);
        p->next = Mini_pools; Mini_pools = p;
      }
    }
  }
  if (p) p->used++;
  pthread_mutex_unlock(&Mini_registry_lock);
  return p;
}

static struct rmshared *rm_new(int L, int M);
static void rm_unref(struct rmshared *rs);
static int mini_create_input(struct filter_in *master, int L, int M, enum filtertype in_type) {
  int const N = L + M - 1;
  bool const real = in_type == REAL;
  int const bins = real ? N / 2 + 1 : N;
  struct minictx *c = calloc(1, sizeof *c);
  if (!c) return -1;
  c->kind = CTX_MINI; c->master = master;
  if (real && (c->rs = rm_new(L, M)) == NULL) { free(c); return -1; }
  size_t const ring_bytes = page_round((size_t)ND * N * (real ? sizeof(float) : sizeof(float complex)));      /* src/filter.c:237,253 */
  void *ring = ring_map(ring_bytes);
  void *fd[ND] = {NULL, NULL, NULL, NULL};
  bool ok = ring != NULL;
  for (int i = 0; ok && i < ND; i++) ok = (fd[i] = lmalloc(sizeof(float complex) * (size_t)N)) != NULL;
  if (!ok) { for (int i = 0; i < ND; i++) free(fd[i]); ring_unmap(&ring, ring_bytes); if (c->rs) rm_unref(c->rs); free(c); return -1; }
  master->points = N; master->bins = bins; master->ilen = L; master->impulse_length = M;
  master->perform_inline = true;                                 /* a mini has no asynchronous half */
  for (int i = 0; i < ND; i++) {
    memset(fd[i], 0, sizeof(float complex) * (size_t)N);
    master->fdomain[i] = fd[i];                                   /* nobody reads a filter2 master's spectrum; kept allocated and zero */
    master->completed_jobs[i] = UINT_MAX;
  }
  if (!master->init) { pthread_mutex_init(&master->filter_mutex, NULL); pthread_cond_init(&master->filter_cond, NULL); master->init = true; }
  master->owner = pthread_self();
  master->in_type = in_type;
  master->input_buffer_size = ring_bytes;
  master->input_buffer = ring;
  memset(ring, 0, ring_bytes);
  if (real) {                                                     /* src/filter.c:258-261 */
    master->input_read_pointer.r = master->input_buffer;
    master->input_write_pointer.r = master->input_read_pointer.r + (M - 1);
    master->input_read_pointer.c = NULL; master->input_write_pointer.c = NULL;
  } else {                                                        /* src/filter.c:243-246 */
    master->input_read_pointer.c = master->input_buffer;
    master->input_write_pointer.c = master->input_read_pointer.c + (M - 1);
    master->input_read_pointer.r = NULL; master->input_write_pointer.r = NULL;
  }
  master->wcnt = 0; master->next_jobnum = 0;
  master->fwd_plan = (fftwf_plan)(void *)c;
  return 0;
}

static void mini_free_input(struct filter_in *master) {           /* the ctx and buffers of a mini master */
  struct minictx *mc = (struct minictx *)(void *)master->fwd_plan;
  if (mc && mc->rs) rm_unref(mc->rs);                              /* (slaves deleted after their master, src/wfm.c:290-293, hold it until they go) */
  free(mc); master->fwd_plan = NULL;
  ring_unmap(&master->input_buffer, master->input_buffer_size);
  for (int i = 0; i < ND; i++) { free(master->fdomain[i]); master->fdomain[i] = NULL; }
}

static int mini_create_output(struct filter_out *slave, struct filter_in *master, int len, enum filtertype out_type) {
  if (out_type == SPECTRUM) return 1;                              /* a block clock needs nothing: let the common path set it up */
  if (out_type != COMPLEX || len != master->ilen) {
    /* not what a pooled instance does (a decimating or REAL-output slave).  A master that has not run yet and has no slaves -- the usual
       order: create_filter_input, then its create_filter_output()s -- is simply re-made as a full engine by the caller (returns 2) */
    struct minictx const *mc = (struct minictx const *)(void const *)master->fwd_plan;
    if (!mc->decided && mc->nslaves == 0) return 2;
    fprintf(stderr, "create_filter_output: a %d-point inline master that already serves a same-size slave takes same-size COMPLEX slaves only (asked: olen %d, type %d)\n",
            master->points, len, (int)out_type);
    return -1;
  }
  struct minipool *p = mini_pool_for(master->ilen, master->impulse_length);
  if (!p) return -1;
  int inst = chz_mini_add(p->h);
  struct msctx *sc = calloc(1, sizeof *sc);
  float complex *buf = lmalloc(sizeof(float complex) * (size_t)master->points);
  float complex *fdom = lmalloc(sizeof(float complex) * (size_t)master->points);
  if (inst < 0 || !sc || !buf || !fdom) {
    if (inst >= 0) chz_mini_release(p->h, inst);
    pthread_mutex_lock(&Mini_registry_lock); p->used--; pthread_mutex_unlock(&Mini_registry_lock);
    free(sc); free(buf); free(fdom);
    return -1;
  }
  sc->kind = CTX_MSLAVE; sc->pool = p; sc->inst = inst;
  ((struct minictx *)(void *)master->fwd_plan)->nslaves++;
  __atomic_store_n(&((struct minictx *)(void *)master->fwd_plan)->decided, true, __ATOMIC_RELEASE);      /* (read without the mutex by execute_filter_input) */
  memset(buf, 0, sizeof(float complex) * (size_t)master->points);
  slave->bins = master->points;                                    /* src/filter.c:346 */
  slave->fdomain = fdom;
  slave->output_buffer.c = buf;
  slave->output.c = buf + slave->bins - len;                       /* src/filter.c:357 */
  slave->rev_plan = (fftwf_plan)(void *)sc;
  return 0;
}

static void mini_delete_output(struct filter_out *slave) {
  struct msctx *sc = (struct msctx *)(void *)slave->rev_plan;
  if (!sc) return;
  chz_mini_release(sc->pool->h, sc->inst);
  pthread_mutex_lock(&Mini_registry_lock); sc->pool->used--; pthread_mutex_unlock(&Mini_registry_lock);
  if (is_mini_master(slave->master)) ((struct minictx *)(void *)slave->master->fwd_plan)->nslaves--;       /* (a master deleted first is all zeros) */
  free(sc);
  slave->rev_plan = NULL;
}

static int mini_execute_input(struct filter_in *f) {
  struct minictx *c = (struct minictx *)(void *)f->fwd_plan;
  unsigned const job = __atomic_fetch_add(&f->next_jobnum, 1u, __ATOMIC_RELAXED);   /* src/filter.c:607; read lock-free by slaves being created */
  int const slot = (int)(job % ND);
  /* readers pick this up without a lock, possibly while a later lap overwrites it (as in the reference): tear-free accesses */
  __atomic_store_n(&f->samples_by_job[slot], f->sample_index, __ATOMIC_RELAXED);   /* src/filter.c:614-615 */
  f->sample_index += (uint64_t)f->ilen;
  if (f->in_type == REAL) {
    c->job_win[slot] = f->input_read_pointer.r;                    /* N contiguous samples: the mirror sees to that */
    f->input_read_pointer.r += f->ilen;                            /* src/filter.c:626-636 */
    ring_wrap((void **)&f->input_read_pointer.r, f->input_buffer, f->input_buffer_size);
  } else {
    c->job_win[slot] = f->input_read_pointer.c;
    f->input_read_pointer.c += f->ilen;
    ring_wrap((void **)&f->input_read_pointer.c, f->input_buffer, f->input_buffer_size);
  }
  pthread_mutex_lock(&f->filter_mutex);
  __atomic_store_n(&f->owner, pthread_self(), __ATOMIC_RELEASE);      /* read without the mutex by execute_filter_output */
  __atomic_store_n(&f->completed_jobs[slot], job, __ATOMIC_RELEASE);
  pthread_cond_broadcast(&f->filter_cond);
  pthread_mutex_unlock(&f->filter_mutex);
  futex_wake_all(&f->completed_jobs[slot]);
  return 0;
}

static int mini_execute_output(struct filter_out *slave, int shift, int slot) {
  struct msctx *sc = (struct msctx *)(void *)slave->rev_plan;
  struct minictx *c = (struct minictx *)(void *)slave->master->fwd_plan;
  struct minipool *p = sc->pool;
  struct mini_req req = {.inst = sc->inst, .shift = shift, .isb = slave->isb ? 1 : 0,
                         .win = (const float *)c->job_win[slot], .out = (float *)slave->output.c};
  pthread_mutex_lock(&p->lock);
  if (p->tail) p->tail->next = &req; else p->head = &req;
  p->tail = &req;
  if (!p->leader) {
    p->leader = true;
    while (p->head) {
      struct mini_req *list = p->head;
      p->head = p->tail = NULL;
      pthread_mutex_unlock(&p->lock);
      int n = 0;
      for (struct mini_req *r = list; r; r = r->next) n++;
      int *inst = malloc(sizeof(int) * (size_t)n * 2);
      const float **win = malloc(sizeof(float *) * (size_t)n * 2);
      unsigned char *isb = malloc((size_t)n);
      int rc = (inst && win && isb) ? 0 : -1;
      if (rc == 0) {
        int *sh = inst + n; float **out = (float **)(win + n);
        int i = 0;
        for (struct mini_req *r = list; r; r = r->next, i++) { inst[i] = r->inst; sh[i] = r->shift; isb[i] = r->isb; win[i] = r->win; out[i] = r->out; }
        rc = chz_mini_execute(p->h, n, inst, win, sh, isb, out);
        if (rc != 0) fprintf(stderr, "execute_filter_output (inline master): %s\n", chz_last_error());
      }
      free(inst); free(win); free(isb);
      pthread_mutex_lock(&p->lock);
      for (struct mini_req *r = list; r;) { struct mini_req *nx = r->next; r->rc = rc; r->done = true; r = nx; }   /* r may vanish once done */
      pthread_cond_broadcast(&p->cv);
    }
    p->leader = false;
  } else {
    while (!req.done) pthread_cond_wait(&p->cv, &p->lock);
  }
  pthread_mutex_unlock(&p->lock);
  return req.rc == 0 ? 0 : -1;
}

/* ---- pooled REAL masters with decimating slaves (chz_rmini_*) -------------------------------------------------------------------
 * struct rmshared is what a master and its slaves share; it is reference-counted because wfm deletes its composite master BEFORE the
 * three slaves (src/wfm.c:290-293) and because the pool instance covers all of them.
 *   create_filter_output  registers the slave (host buffers only).  A slave the pool cannot serve -- a fifth one, a block size outside
 *                         chz_rmini_create's limits -- turns a master that has not run into a full engine in place, its registered
 *                         slaves with it (rmini_to_engine); on a master that has run it fails loudly.  A master whose first block
 *                         arrives before any slave (a front end; a SPECTRUM-only use) becomes an engine too (execute_filter_input).
 *   execute_filter_output the first one joins the pool of the geometry.  A request runs ALL slaves of the instance, each with the shift
 *                         it was last executed with; the siblings' outputs are kept with (job, shift, ISB flag, response epoch), and a
 *                         sibling's execute_filter_output for the same job and shift copies them out without a device round trip (wfm:
 *                         mono, then pilot, then L-R, constant shifts).  Anything else is a fresh request; the kernel is stateless, so
 *                         both ways give the same bits.  Requests go through a batch-leader queue like mini_execute_output's: one
 *                         launch serves every thread that arrived meanwhile.  A block on which no slave executes costs nothing. */
struct rmini_req {
  int inst;
  const float *win;
  int shift[RM_MAX];
  unsigned char isb[RM_MAX], mask;
  float *out[RM_MAX];
  int rc;
  bool done;
  struct rmini_req *next;
};
struct rminipool {
  int L, M, ns, olen[RM_MAX], type[RM_MAX], cap, used;
  chz_rmini *h;
  pthread_mutex_t lock;
  pthread_cond_t cv;
  struct rmini_req *head, *tail;
  bool leader;
  struct rminipool *next;
};
struct rmshared {
  pthread_mutex_t lock;             /* held across a request: a sibling arriving meanwhile finds its prefetched block afterwards */
  int refs;                         /* the master + every registered slave not yet deleted */
  int L, M, nsl;
  struct filter_out *slv[RM_MAX];   /* in creation order = the pool's slave order; NULL once deleted */
  int olen[RM_MAX], type[RM_MAX];
  bool joined;
  struct rminipool *pool; int inst;
  int last_shift[RM_MAX];
  unsigned epoch[RM_MAX];           /* bumped by set_filter */
  void *pf[RM_MAX];                 /* prefetched output of each slave: olen samples */
  bool pf_valid[RM_MAX];
  unsigned pf_job[RM_MAX], pf_epoch[RM_MAX];
  int pf_shift[RM_MAX];
  unsigned char pf_isb[RM_MAX];
};
struct rsctx {                      /* hangs off slave->rev_plan */
  int kind;                         /* CTX_RSLAVE */
  struct rmshared *sh;
  int idx;
};

static int Pool_real_masters;       /* ka9q_hip_pool_real_masters() */
static struct rminipool *Rmini_pools;

static bool rmini_available(void) {
  return chz_rmini_create && chz_rmini_destroy && chz_rmini_check && chz_rmini_add && chz_rmini_release && chz_rmini_set_response && chz_rmini_execute;
}
static bool rmini_wanted(int L, int M, enum filtertype in_type) {
  if (!__atomic_load_n(&Pool_real_masters, __ATOMIC_RELAXED) || !rmini_available() || in_type != REAL) return false;
  long const N = (long)L + M - 1;
  return !(N & 1) && N >= 16 && N <= 16384;
}
/* would the pool of the geometry with this slave added exist?  The engine library answers (chz_rmini_check: chz_rmini_create's own
   limits, no device touched), so that what the pool would refuse is known when the slave is created, while the master can still
   become an engine */
static bool rmini_serves(struct rmshared const *rs, int len, enum filtertype out_type) {
  if (rs->nsl >= RM_MAX || (out_type != COMPLEX && out_type != REAL)) return false;
  int olen[RM_MAX], type[RM_MAX];
  for (int s = 0; s < rs->nsl; s++) { olen[s] = rs->olen[s]; type[s] = rs->type[s]; }
  olen[rs->nsl] = len; type[rs->nsl] = out_type == REAL ? CHZ_REAL : CHZ_COMPLEX;
  return chz_rmini_check(rs->L, rs->M, rs->nsl + 1, olen, type) == 0;
}
static struct rmshared *rm_new(int L, int M) {
  struct rmshared *rs = calloc(1, sizeof *rs);
  if (!rs) return NULL;
  pthread_mutex_init(&rs->lock, NULL);
  rs->refs = 1; rs->L = L; rs->M = M;
  return rs;
}
static void rm_unref(struct rmshared *rs) {
  pthread_mutex_lock(&rs->lock);
  int const left = --rs->refs;
  pthread_mutex_unlock(&rs->lock);
  if (left > 0) return;
  if (rs->joined) {
    chz_rmini_release(rs->pool->h, rs->inst);
    pthread_mutex_lock(&Mini_registry_lock); rs->pool->used--; pthread_mutex_unlock(&Mini_registry_lock);
  }
  for (int s = 0; s < RM_MAX; s++) free(rs->pf[s]);
  pthread_mutex_destroy(&rs->lock);
  free(rs);
}
static bool is_rmini_slave(const struct filter_out *slave) {
  return slave && slave->rev_plan && *(const int *)(const void *)slave->rev_plan == CTX_RSLAVE;
}

/* 0: registered; 1: a block clock, nothing to do; 2: not what the pool serves and the master has not run -- make it an engine; -1: refused */
static int rmini_create_output(struct filter_out *slave, struct filter_in *master, int len, enum filtertype out_type) {
  if (out_type == SPECTRUM) return 1;
  struct minictx *mc = (struct minictx *)(void *)master->fwd_plan;
  struct rmshared *rs = mc->rs;
  bool const ran = __atomic_load_n(&master->next_jobnum, __ATOMIC_RELAXED) != 0;
  pthread_mutex_lock(&rs->lock);
  bool const fits = !rs->joined && !ran && rmini_serves(rs, len, out_type);
  pthread_mutex_unlock(&rs->lock);
  if (!fits) {
    if (!ran) return 2;
    fprintf(stderr, "create_filter_output: a pooled %d-point REAL master that has run takes no new slaves (asked: olen %d, type %d); create them before its first block\n",
            master->points, len, (int)out_type);
    return -1;
  }
  bool const real = out_type == REAL;
  struct rsctx *sc = calloc(1, sizeof *sc);
  slave->bins = real ? slave->points / 2 + 1 : slave->points;      /* src/filter.c:346,374 */
  slave->fdomain = lmalloc(sizeof(float complex) * (size_t)slave->bins);
  void *pf = malloc((real ? sizeof(float) : sizeof(float complex)) * (size_t)len);
  if (real) {
    slave->output_buffer.r = lmalloc(sizeof(float) * (size_t)slave->points);
    if (slave->output_buffer.r) { memset(slave->output_buffer.r, 0, sizeof(float) * (size_t)slave->points); slave->output.r = slave->output_buffer.r + slave->points - len; }
  } else {
    slave->output_buffer.c = lmalloc(sizeof(float complex) * (size_t)slave->points);
    if (slave->output_buffer.c) { memset(slave->output_buffer.c, 0, sizeof(float complex) * (size_t)slave->points); slave->output.c = slave->output_buffer.c + slave->bins - len; }
  }
  if (!sc || !pf || !slave->fdomain || (!slave->output_buffer.c && !slave->output_buffer.r)) {
    free(sc); free(pf); FREE(slave->fdomain); FREE(slave->output_buffer.c); FREE(slave->output_buffer.r);
    return -1;
  }
  pthread_mutex_lock(&rs->lock);
  int const k = rs->nsl++;
  rs->slv[k] = slave; rs->olen[k] = len; rs->type[k] = real ? CHZ_REAL : CHZ_COMPLEX; rs->pf[k] = pf; rs->refs++;
  pthread_mutex_unlock(&rs->lock);
  sc->kind = CTX_RSLAVE; sc->sh = rs; sc->idx = k;
  slave->rev_plan = (fftwf_plan)(void *)sc;
  __atomic_store_n(&mc->decided, true, __ATOMIC_RELEASE);          /* (a first block with no slave at all makes an engine of it: execute_filter_input) */
  return 0;
}

static void rmini_delete_output(struct filter_out *slave) {        /* never looks at slave->master: it may be gone (src/wfm.c:290-293) */
  struct rsctx *sc = (struct rsctx *)(void *)slave->rev_plan;
  struct rmshared *rs = sc->sh;
  pthread_mutex_lock(&rs->lock);
  rs->slv[sc->idx] = NULL; rs->pf_valid[sc->idx] = false;
  pthread_mutex_unlock(&rs->lock);
  rm_unref(rs);
  free(sc);
  slave->rev_plan = NULL;
}

static int rmini_set_response(struct filter_out *slave, const float complex *response) {
  struct rsctx *sc = (struct rsctx *)(void *)slave->rev_plan;
  struct rmshared *rs = sc->sh;
  int rc = 0;
  pthread_mutex_lock(&rs->lock);
  rs->epoch[sc->idx]++;
  if (rs->joined) rc = chz_rmini_set_response(rs->pool->h, rs->inst, sc->idx, (const float *)response);
  pthread_mutex_unlock(&rs->lock);
  if (rc != 0) fprintf(stderr, "set_filter: %s\n", chz_last_error());
  return rc == 0 ? 0 : -1;
}

/* a pool of this geometry with a free instance (created on demand) */
static struct rminipool *rmini_pool_for(struct rmshared const *rs) {
  pthread_mutex_lock(&Mini_registry_lock);
  struct rminipool *p = Rmini_pools;
  for (; p; p = p->next) {
    bool same = p->L == rs->L && p->M == rs->M && p->ns == rs->nsl && p->used < p->cap;
    for (int s = 0; same && s < rs->nsl; s++) same = p->olen[s] == rs->olen[s] && p->type[s] == rs->type[s];
    if (same) break;
  }
  if (!p) {
    p = calloc(1, sizeof *p);
    if (p) {
      const char *dev = getenv("KA9Q_HIP_DEVICE");
      p->L = rs->L; p->M = rs->M; p->ns = rs->nsl; p->cap = 256;
      for (int s = 0; s < rs->nsl; s++) { p->olen[s] = rs->olen[s]; p->type[s] = rs->type[s]; }
      if (chz_rmini_create(&p->h, p->L, p->M, p->ns, p->olen, p->type, p->cap, dev ? atoi(dev) : 0) != 0) {
        fprintf(stderr, "filter_hip: REAL inline-master pool L=%d M=%d (%d slaves): %s\n", p->L, p->M, p->ns, chz_last_error());
        free(p); p = NULL;
      } else {
        pthread_mutex_init(&p->lock, NULL);
        pthread_cond_init(&p->cv, NULL);
        p->next = Rmini_pools; Rmini_pools = p;
      }
    }
  }
  if (p) p->used++;
  pthread_mutex_unlock(&Mini_registry_lock);
  return p;
}
/* the slave list is final: take an instance and hand it the responses set so far (caller holds rs->lock) */
static int rmini_join(struct rmshared *rs) {
  struct rminipool *p = rmini_pool_for(rs);
  if (!p) return -1;
  int const inst = chz_rmini_add(p->h);
  if (inst < 0) {
    fprintf(stderr, "filter_hip: REAL inline-master pool: %s\n", chz_last_error());
    pthread_mutex_lock(&Mini_registry_lock); p->used--; pthread_mutex_unlock(&Mini_registry_lock);
    return -1;
  }
  rs->pool = p; rs->inst = inst; rs->joined = true;
  for (int s = 0; s < rs->nsl; s++) {
    struct filter_out *o = rs->slv[s];
    if (!o) continue;
    pthread_mutex_lock(&o->response_mutex);
    int const rc = o->response ? chz_rmini_set_response(p->h, inst, s, (const float *)o->response) : 0;
    pthread_mutex_unlock(&o->response_mutex);
    if (rc != 0) {                                                 /* not joined after all: the next execute_filter_output tries again */
      fprintf(stderr, "filter_hip: REAL inline-master pool: %s\n", chz_last_error());
      rs->joined = false; rs->pool = NULL;
      chz_rmini_release(p->h, inst);
      pthread_mutex_lock(&Mini_registry_lock); p->used--; pthread_mutex_unlock(&Mini_registry_lock);
      return -1;
    }
  }
  return 0;
}

/* queue one request for the pool's next launch; the first thread to arrive leads (see mini_execute_output) */
static int rmini_run(struct rminipool *p, struct rmini_req *req) {
  pthread_mutex_lock(&p->lock);
  if (p->tail) p->tail->next = req; else p->head = req;
  p->tail = req;
  if (!p->leader) {
    p->leader = true;
    while (p->head) {
      struct rmini_req *list = p->head;
      p->head = p->tail = NULL;
      pthread_mutex_unlock(&p->lock);
      int n = 0;
      for (struct rmini_req *r = list; r; r = r->next) n++;
      size_t const ns = (size_t)p->ns;
      int *inst = malloc(sizeof(int) * (size_t)n * (1 + ns));
      const float **win = malloc(sizeof(float *) * (size_t)n * (1 + ns));
      unsigned char *flags = malloc((size_t)n * (1 + ns));
      int rc = (inst && win && flags) ? 0 : -1;
      if (rc == 0) {
        int *sh = inst + n; float **out = (float **)(win + n);
        unsigned char *mask = flags, *isb = flags + n;
        size_t i = 0;
        for (struct rmini_req *r = list; r; r = r->next, i++) {
          inst[i] = r->inst; win[i] = r->win; mask[i] = r->mask;
          for (size_t s = 0; s < ns; s++) { sh[i * ns + s] = r->shift[s]; isb[i * ns + s] = r->isb[s]; out[i * ns + s] = r->out[s]; }
        }
        rc = chz_rmini_execute(p->h, n, inst, win, sh, mask, isb, out);
        if (rc != 0) fprintf(stderr, "execute_filter_output (pooled REAL master): %s\n", chz_last_error());
      }
      free(inst); free(win); free(flags);
      pthread_mutex_lock(&p->lock);
      for (struct rmini_req *r = list; r;) { struct rmini_req *nx = r->next; r->rc = rc; r->done = true; r = nx; }   /* r may vanish once done */
      pthread_cond_broadcast(&p->cv);
    }
    p->leader = false;
  } else {
    while (!req->done) pthread_cond_wait(&p->cv, &p->lock);
  }
  pthread_mutex_unlock(&p->lock);
  return req->rc == 0 ? 0 : -1;
}

static int rmini_execute_output(struct filter_out *slave, int shift, int slot, unsigned job) {
  struct rsctx *sc = (struct rsctx *)(void *)slave->rev_plan;
  struct rmshared *rs = sc->sh;
  struct minictx *c = (struct minictx *)(void *)slave->master->fwd_plan;
  int const k = sc->idx;
  bool const real = slave->out_type == REAL;
  void *const dst = real ? (void *)slave->output.r : (void *)slave->output.c;
  size_t const bytes = (real ? sizeof(float) : sizeof(float complex)) * (size_t)slave->olen;
  unsigned char const isb = (!real && slave->isb) ? 1 : 0;
  pthread_mutex_lock(&rs->lock);
  if (!rs->joined && rmini_join(rs) != 0) { pthread_mutex_unlock(&rs->lock); return -1; }
  if (rs->pf_valid[k] && rs->pf_job[k] == job && rs->pf_shift[k] == shift && rs->pf_isb[k] == isb && rs->pf_epoch[k] == rs->epoch[k]) {
    memcpy(dst, rs->pf[k], bytes);                                 /* computed by a sibling's request for this very block */
    rs->pf_valid[k] = false;
    pthread_mutex_unlock(&rs->lock);
    return 0;
  }
  rs->last_shift[k] = shift;
  struct rmini_req req = {.inst = rs->inst, .win = (const float *)c->job_win[slot]};
  for (int s = 0; s < rs->nsl; s++) {
    struct filter_out *o = rs->slv[s];
    if (!o || (s != k && __atomic_load_n(&o->response, __ATOMIC_ACQUIRE) == NULL)) continue;
    req.mask |= (unsigned char)(1u << s);
    req.shift[s] = rs->last_shift[s];
    req.isb[s] = s == k ? isb : (unsigned char)((o->out_type == COMPLEX && o->isb) ? 1 : 0);
    req.out[s] = s == k ? (float *)dst : (float *)rs->pf[s];
    rs->pf_valid[s] = false;
  }
  int const rc = rmini_run(rs->pool, &req);
  if (rc == 0)
    for (int s = 0; s < rs->nsl; s++)
      if (s != k && ((req.mask >> s) & 1)) {
        rs->pf_valid[s] = true; rs->pf_job[s] = job; rs->pf_shift[s] = req.shift[s]; rs->pf_isb[s] = req.isb[s]; rs->pf_epoch[s] = rs->epoch[s];
      }
  pthread_mutex_unlock(&rs->lock);
  return rc;
}
