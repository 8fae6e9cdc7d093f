/* jni/demi_jni.c — the JNI shim between DEMi's Scala adapter (scala/akka/dispatch/verification/gpu/DemiGpu.scala) and the
 * C ABI of libdemi_gpu.so (include/demi_gpu.h).  One Java_..._DemiGpu_<name> per entry point, nothing but marshalling.
 *
 * Marshalling rules (round 3):
 *   - small structs travel as int / long arrays in field order and are COPIED with Get/Set<Type>ArrayRegion;
 *   - bulk buffers are accessed with Get<Type>ArrayElements / Release<Type>ArrayElements.  NOT GetPrimitiveArrayCritical: an
 *     entry point may run a whole exploration, compile a table with hiprtc, start host thread pools or take part in an
 *     RCCL collective, and a JNI critical region must neither block nor last (it holds off the collector);
 *   - every array length is checked against what the C entry point reads or writes BEFORE the call: a mismatched caller gets
 *     DEMI_ERR_INVALID_ARG instead of a corrupted Java heap;
 *   - a non-null array whose Get<Type>ArrayElements returns NULL (the JVM is out of memory, an exception is pending) is an
 *     error, never "absent": NULL means something to the C ABI (no conjoined atoms, no masks), so passing it on would silently
 *     change the call (LOST below);
 *   - JNI_OnLoad refuses a libdemi_gpu.so of another struct-layout generation (demi_abi_version() != DEMI_ABI_VERSION).
 * Build: make -C jni (needs JAVA_HOME; without a JDK `make -C jni check` compiles against jni/stub/jni.h).
 *
 * Array conventions (little-endian, same layouts as the C structs):
 *   events    byte[8 * n]     demi_ext_event          recorded  byte[16 * n]  demi_rec_event
 *   verdicts  long[2 * n]     demi_verdict (long 0 = flags | fingerprint << 32, long 1 = hash)
 *   masks     long[4 * n]     candidate subsequences  violations long[2 * n]  demi_violation (index, fingerprint | flags << 32)
 *   limits    int[9]          demi_limits             dporParams int[7]  demi_dpor_params     dporSearch int[9]  demi_dpor_search
 *   dporStats long[13]        demi_dpor_stats (kernel_ms as raw double bits; fetches last)                                       */
#include <jni.h>
#include <stdint.h>
#include <string.h>

#include "demi_gpu.h"

#define FN(name) Java_akka_dispatch_verification_gpu_DemiGpu_##name
#define CTX(h) ((demi_ctx*)(intptr_t)(h))
#define LEN(arr) ((arr) ? (int64_t)(*e)->GetArrayLength(e, (arr)) : (int64_t)-1)
/* bulk buffers (may be NULL where the C ABI takes NULL) */
#define BYTES(arr) ((arr) ? (void*)(*e)->GetByteArrayElements(e, (arr), NULL) : NULL)
#define SHORTS(arr) ((arr) ? (void*)(*e)->GetShortArrayElements(e, (arr), NULL) : NULL)
#define INTS(arr) ((arr) ? (void*)(*e)->GetIntArrayElements(e, (arr), NULL) : NULL)
#define LONGS(arr) ((arr) ? (void*)(*e)->GetLongArrayElements(e, (arr), NULL) : NULL)
#define LOST(arr, p) ((arr) != NULL && (p) == NULL)     /* the array exists and its elements could not be obtained */
/* Results go back through Set*ArrayRegion.  When a Get*ArrayElements failed (LOST) an OutOfMemoryError is pending, and with an
 * exception pending JNI allows only a short list of calls - the Release* calls among them, Set*ArrayRegion not (-Xcheck:jni
 * aborts on it): the outputs are skipped then, the caller sees the exception and DEMI_ERR_INVALID_ARG. */
#define SET_LONGS(arr, n, src) do { if (!(*e)->ExceptionCheck(e)) (*e)->SetLongArrayRegion(e, (arr), 0, (n), (src)); } while (0)
#define PUT_BYTES(arr, p, mode) do { if ((arr) && (p)) (*e)->ReleaseByteArrayElements(e, (arr), (jbyte*)(p), (mode)); } while (0)
#define PUT_SHORTS(arr, p, mode) do { if ((arr) && (p)) (*e)->ReleaseShortArrayElements(e, (arr), (jshort*)(p), (mode)); } while (0)
#define PUT_INTS(arr, p, mode) do { if ((arr) && (p)) (*e)->ReleaseIntArrayElements(e, (arr), (jint*)(p), (mode)); } while (0)
#define PUT_LONGS(arr, p, mode) do { if ((arr) && (p)) (*e)->ReleaseLongArrayElements(e, (arr), (jlong*)(p), (mode)); } while (0)

JNIEXPORT jint JNICALL JNI_OnLoad(JavaVM* vm, void* reserved) {
  (void)vm; (void)reserved;
  /* a library built from another generation of demi_gpu.h would read these arrays with other struct layouts */
  return demi_abi_version() == DEMI_ABI_VERSION ? JNI_VERSION_1_6 : JNI_ERR;
}

/* demi_limits from int[9] (a shorter array of an older adapter is refused, not read out of bounds) */
static int limits_of(JNIEnv* e, jintArray limits, demi_limits* x) {
  jint l[9];
  if (LEN(limits) != 9) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, limits, 0, 9, l);
  x->max_messages = (uint32_t)l[0]; x->invariant_check_interval = (uint32_t)l[1]; x->p_max = (uint32_t)l[2];
  x->looking_for_valid = (uint32_t)l[3]; x->looking_for = (uint32_t)l[4]; x->populate_all = (uint32_t)l[5]; x->strategy = (uint32_t)l[6];
  x->filter_known_absents = (uint32_t)l[7]; x->executions_per_instance = (uint32_t)l[8];
  return DEMI_OK;
}
static int dpor_params_of(JNIEnv* e, jintArray params, demi_dpor_params* x) {
  jint p[7];
  if (LEN(params) != 7) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 7, p);
  x->depth_bound = (uint32_t)p[0]; x->max_messages = (uint32_t)p[1]; x->looking_for_valid = (uint32_t)p[2]; x->looking_for = (uint32_t)p[3];
  x->p_max = (uint32_t)p[4]; x->max_pairs = (uint32_t)p[5]; x->prioritize_pending = (uint32_t)p[6];
  return DEMI_OK;
}

JNIEXPORT jlong JNICALL FN(ctxCreate)(JNIEnv* e, jclass c, jint device) {
  demi_ctx* ctx = NULL;
  (void)e; (void)c;
  return demi_ctx_create(device, &ctx) == DEMI_OK ? (jlong)(intptr_t)ctx : 0;
}
JNIEXPORT void JNICALL FN(ctxDestroy)(JNIEnv* e, jclass c, jlong h) { (void)e; (void)c; demi_ctx_destroy(CTX(h)); }
JNIEXPORT jstring JNICALL FN(lastError)(JNIEnv* e, jclass c, jlong h) { (void)c; return (*e)->NewStringUTF(e, demi_last_error(CTX(h))); }

/* demi_model_load: inv = { inv_kind, inv_fa, inv_va, inv_fb, fp_match_mask [, flags (DEMI_MODEL_WIDE)] } */
JNIEXPORT jint JNICALL FN(modelLoad)(JNIEnv* e, jclass c, jlong h, jint nActors, jbyteArray msgClass, jbyteArray actorClass,
                                     jint nClasses, jshortArray handlerStart, jintArray code, jlongArray initState, jintArray inv) {
  demi_model m;
  jint iv[6] = {0, 0, 0, 0, 0, 0};
  (void)c;
  memset(&m, 0, sizeof m);
  const int64_t n_inv = LEN(inv), n_types = LEN(msgClass);
  if (n_inv < 5 || n_inv > 6 || n_types < 1 || nActors < 1 || nClasses < 1) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, inv, 0, (jsize)n_inv, iv);
  m.n_actors = (uint32_t)nActors; m.n_classes = (uint32_t)nClasses;
  m.n_msg_types = (uint32_t)n_types;
  m.code_len = (uint32_t)(LEN(code) < 0 ? 0 : LEN(code));
  m.inv_kind = (uint32_t)iv[0]; m.inv_fa = (uint32_t)iv[1]; m.inv_va = (uint32_t)iv[2]; m.inv_fb = (uint32_t)iv[3];
  m.fp_match_mask = (uint32_t)iv[4];
  m.flags = (uint32_t)iv[5];                             /* a wide model: initState holds two words per actor */
  /* what demi_model_load reads: actor_class[n_actors], handler_start[n_classes * n_msg_types], init_state[n_actors (x 2 wide)] */
  if (LEN(actorClass) < nActors || LEN(handlerStart) < (int64_t)nClasses * n_types ||
      LEN(initState) < (int64_t)nActors * ((m.flags & DEMI_MODEL_WIDE) ? 2 : 1) || LEN(code) < 0)
    return DEMI_ERR_INVALID_ARG;
  m.msg_class = (const uint8_t*)BYTES(msgClass);
  m.actor_class = (const uint8_t*)BYTES(actorClass);
  m.handler_start = (const uint16_t*)SHORTS(handlerStart);
  m.code = (const uint32_t*)INTS(code);
  m.init_state = (const uint64_t*)LONGS(initState);
  jint rc = (LOST(msgClass, m.msg_class) || LOST(actorClass, m.actor_class) || LOST(handlerStart, m.handler_start) || LOST(code, m.code) ||
             LOST(initState, m.init_state)) ? DEMI_ERR_INVALID_ARG : demi_model_load(CTX(h), &m);
  PUT_LONGS(initState, m.init_state, JNI_ABORT);
  PUT_INTS(code, m.code, JNI_ABORT);
  PUT_SHORTS(handlerStart, m.handler_start, JNI_ABORT);
  PUT_BYTES(actorClass, m.actor_class, JNI_ABORT);
  PUT_BYTES(msgClass, m.msg_class, JNI_ABORT);
  return rc;
}
JNIEXPORT jint JNICALL FN(modelSpecialize)(JNIEnv* e, jclass c, jlong h, jboolean enable) {
  (void)e; (void)c;
  return demi_model_specialize(CTX(h), enable ? 1 : 0);
}
JNIEXPORT jint JNICALL FN(traceLoad)(JNIEnv* e, jclass c, jlong h, jbyteArray events) {
  (void)c;
  const int64_t len = LEN(events);
  if (len < 0 || len % 8) return DEMI_ERR_INVALID_ARG;
  void* p = BYTES(events);
  jint rc = LOST(events, p) ? DEMI_ERR_INVALID_ARG : demi_trace_load(CTX(h), (const demi_ext_event*)p, (uint32_t)(len / 8));
  PUT_BYTES(events, p, JNI_ABORT);
  return rc;
}

/* demi_ext_payload_areas: the payload areas of the external events the next traceLoad / dporLoad loads (null: forget) */
JNIEXPORT jint JNICALL FN(extPayloadAreas)(JNIEnv* e, jclass c, jlong h, jlongArray areas) {
  (void)c;
  if (!areas) return demi_ext_payload_areas(CTX(h), NULL, 0);
  const int64_t len = LEN(areas);
  if (len < 0 || len > DEMI_MAX_EXT_EVENTS) return DEMI_ERR_INVALID_ARG;
  void* p = LONGS(areas);
  jint rc = LOST(areas, p) ? DEMI_ERR_INVALID_ARG : demi_ext_payload_areas(CTX(h), (const uint64_t*)p, (uint32_t)len);
  PUT_LONGS(areas, p, JNI_ABORT);
  return rc;
}

/* ---- K1 */
JNIEXPORT jint JNICALL FN(randomExplore)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jlong n, jintArray limits, jlongArray verdicts) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || n < 0 || LEN(verdicts) < 2 * (int64_t)n) return DEMI_ERR_INVALID_ARG;
  void* o = LONGS(verdicts);
  jint rc = LOST(verdicts, o) ? DEMI_ERR_INVALID_ARG : demi_random_explore(CTX(h), (uint64_t)seedBase, NULL, (uint64_t)n, &lim, (demi_verdict*)o);
  PUT_LONGS(verdicts, o, 0);
  return rc;
}
/* out: long[2 * cap]; counts: long[2] = { number flagged, lowest flagged index }; flagMask = DEMI_V_* bits */
JNIEXPORT jint JNICALL FN(randomExploreFlagged)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jlong n, jintArray limits, jint flagMask,
                                               jlongArray out, jlongArray counts) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || n < 0 || LEN(out) < 0 || LEN(out) % 2 || LEN(counts) != 2) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(out) / 2);
  uint64_t n_flagged = 0, first = 0;
  void* o = LONGS(out);
  jint rc = LOST(out, o) ? DEMI_ERR_INVALID_ARG
                         : demi_random_explore_flagged(CTX(h), (uint64_t)seedBase, (uint64_t)n, &lim, (uint32_t)flagMask, (demi_violation*)o, cap,
                                                       &n_flagged, &first);
  PUT_LONGS(out, o, 0);
  const jlong cn[2] = {(jlong)n_flagged, (jlong)first};
  SET_LONGS(counts, 2, cn);
  return rc;
}
/* explore() in pieces, two calls in flight in one context.  Returns the ticket (> 0) or a negative demi_status. */
JNIEXPORT jint JNICALL FN(randomExploreSubmit)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jlong n, jintArray limits, jint flagMask) {
  demi_limits lim;
  uint32_t ticket = 0;
  (void)c;
  if (limits_of(e, limits, &lim) || n <= 0) return DEMI_ERR_INVALID_ARG;
  const int rc = demi_random_explore_submit(CTX(h), (uint64_t)seedBase, (uint64_t)n, &lim, (uint32_t)flagMask, 0u, &ticket);
  return rc ? rc : (jint)ticket;
}
/* out: long[2 * cap] (flagged entries, sorted by index); counts: long[2] = { number flagged, lowest flagged index } */
JNIEXPORT jint JNICALL FN(randomExploreWait)(JNIEnv* e, jclass c, jlong h, jint ticket, jlongArray out, jlongArray counts) {
  (void)c;
  if (ticket <= 0 || LEN(out) < 0 || LEN(out) % 2 || LEN(counts) != 2) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(out) / 2);
  uint64_t n_flagged = 0, first = 0;
  void* o = LONGS(out);
  jint rc = LOST(out, o) ? DEMI_ERR_INVALID_ARG
                         : demi_random_explore_wait(CTX(h), (uint32_t)ticket, NULL, (demi_violation*)o, cap, &n_flagged, &first);
  PUT_LONGS(out, o, 0);
  const jlong cn[2] = {(jlong)n_flagged, (jlong)first};
  SET_LONGS(counts, 2, cn);
  return rc;
}
/* verdict: long[2]; recorded: byte[16 * cap]; returns the number of recorded events, or a negative demi_status */
JNIEXPORT jint JNICALL FN(randomGetTrace)(JNIEnv* e, jclass c, jlong h, jlong seed, jintArray limits, jlongArray verdict, jbyteArray recorded) {
  demi_limits lim;
  demi_verdict v;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(verdict) != 2 || LEN(recorded) < 0 || LEN(recorded) % (jint)sizeof(demi_rec_event)) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(recorded) / (jint)sizeof(demi_rec_event));
  uint32_t n_out = 0;
  memset(&v, 0, sizeof v);
  void* r = BYTES(recorded);
  jint rc = LOST(recorded, r) ? DEMI_ERR_INVALID_ARG : demi_random_get_trace(CTX(h), (uint64_t)seed, &lim, &v, (demi_rec_event*)r, cap, &n_out);
  PUT_BYTES(recorded, r, 0);
  SET_LONGS(verdict, 2, (const jlong*)(const void*)&v);
  return rc == DEMI_OK ? (jint)n_out : rc;
}

/* the same for execution number execIndex of the carried-generator instance seeded `seed` */
JNIEXPORT jint JNICALL FN(randomGetTraceCarried)(JNIEnv* e, jclass c, jlong h, jlong seed, jint execIndex, jintArray limits, jlongArray verdict,
                                                jbyteArray recorded) {
  demi_limits lim;
  demi_verdict v;
  (void)c;
  if (limits_of(e, limits, &lim) || execIndex < 0 || LEN(verdict) != 2 || LEN(recorded) < 0 || LEN(recorded) % (jint)sizeof(demi_rec_event)) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(recorded) / (jint)sizeof(demi_rec_event));
  uint32_t n_out = 0, ran = 0;
  memset(&v, 0, sizeof v);
  void* r = BYTES(recorded);
  jint rc = LOST(recorded, r) ? DEMI_ERR_INVALID_ARG
                              : demi_random_get_trace_carried(CTX(h), (uint64_t)seed, (uint32_t)execIndex, &lim, &v, (demi_rec_event*)r, cap, &n_out, &ran);
  PUT_BYTES(recorded, r, 0);
  SET_LONGS(verdict, 2, (const jlong*)(const void*)&v);
  if (rc == DEMI_OK && ran != (uint32_t)execIndex) return DEMI_ERR_INVALID_ARG;      /* an earlier execution of the chain already violated */
  return rc == DEMI_OK ? (jint)n_out : rc;
}

/* ---- K2 */
JNIEXPORT jint JNICALL FN(replayLoad)(JNIEnv* e, jclass c, jlong h, jbyteArray externals, jbyteArray recorded) {
  (void)c;
  const int64_t le = LEN(externals), lr = LEN(recorded);
  if (le < 0 || le % 8 || lr < 0 || lr % (jint)sizeof(demi_rec_event)) return DEMI_ERR_INVALID_ARG;
  void* x = BYTES(externals);
  void* r = BYTES(recorded);
  jint rc = (LOST(externals, x) || LOST(recorded, r)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_load(CTX(h), (const demi_ext_event*)x, (uint32_t)(le / 8), (const demi_rec_event*)r, (uint32_t)(lr / (jint)sizeof(demi_rec_event)));
  PUT_BYTES(recorded, r, JNI_ABORT);
  PUT_BYTES(externals, x, JNI_ABORT);
  return rc;
}
JNIEXPORT jint JNICALL FN(replayBatch)(JNIEnv* e, jclass c, jlong h, jlongArray masks, jintArray limits, jlongArray verdicts) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(masks) < 0 || LEN(masks) % 4) return DEMI_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)(LEN(masks) / 4);
  if (LEN(verdicts) < 2 * (int64_t)n) return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masks);
  void* o = LONGS(verdicts);
  jint rc = (LOST(masks, m) || LOST(verdicts, o)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_batch_sharded(CTX(h), (const uint64_t*)m, n, &lim, (demi_verdict*)o);   /* = demi_replay_batch without a communicator */
  PUT_LONGS(verdicts, o, 0);
  PUT_LONGS(masks, m, JNI_ABORT);
  return rc;
}
/* replayBatch in pieces, two calls in flight in one context (single rank).  masks: long[4 * n], the library's own copy is taken before
 * this returns.  Returns the ticket (> 0) or a negative demi_status. */
JNIEXPORT jint JNICALL FN(replayBatchSubmit)(JNIEnv* e, jclass c, jlong h, jlongArray masks, jintArray limits, jint flagMask,
                                            jboolean wantVerdicts) {
  demi_limits lim;
  uint32_t ticket = 0;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(masks) <= 0 || LEN(masks) % 4) return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masks);
  const int rc = LOST(masks, m) ? DEMI_ERR_INVALID_ARG
                 : demi_replay_batch_submit(CTX(h), (const uint64_t*)m, (uint64_t)(LEN(masks) / 4), &lim, (uint32_t)flagMask,
                                            wantVerdicts ? 1u : 0u, &ticket);
  PUT_LONGS(masks, m, JNI_ABORT);
  return rc ? rc : (jint)ticket;
}
/* n: the candidates of that submit (the library writes n verdicts: the array is checked against the caller's n, which must be the
 * submit's); verdictsOrNull: long[2 * n]; out: long[2 * cap] (flagged entries, sorted by index); counts: long[2] = { number
 * flagged, lowest flagged index } */
JNIEXPORT jint JNICALL FN(replayBatchWait)(JNIEnv* e, jclass c, jlong h, jint ticket, jlong n, jlongArray verdictsOrNull, jlongArray out,
                                          jlongArray counts) {
  (void)c;
  if (ticket <= 0 || n <= 0 || LEN(out) < 0 || LEN(out) % 2 || LEN(counts) != 2) return DEMI_ERR_INVALID_ARG;
  if (verdictsOrNull && LEN(verdictsOrNull) < 2 * (int64_t)n) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(out) / 2);
  uint64_t n_flagged = 0, first = 0;
  void* v = LONGS(verdictsOrNull);
  void* o = LONGS(out);
  jint rc = (LOST(verdictsOrNull, v) || LOST(out, o)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_batch_wait(CTX(h), (uint32_t)ticket, (demi_verdict*)v, (demi_violation*)o, cap, &n_flagged, &first);
  PUT_LONGS(out, o, 0);
  PUT_LONGS(verdictsOrNull, v, 0);
  const jlong cn[2] = {(jlong)n_flagged, (jlong)first};
  SET_LONGS(counts, 2, cn);
  return rc;
}
JNIEXPORT jint JNICALL FN(replayRemovalBatch)(JNIEnv* e, jclass c, jlong h, jlongArray masksOrNull, jintArray skip, jintArray limits,
                                             jlongArray verdicts) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(skip) < 0) return DEMI_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)LEN(skip);
  if (LEN(verdicts) < 2 * (int64_t)n || (masksOrNull && LEN(masksOrNull) < 4 * (int64_t)n)) return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masksOrNull);
  void* s = INTS(skip);
  void* o = LONGS(verdicts);
  jint rc = (LOST(masksOrNull, m) || LOST(skip, s) || LOST(verdicts, o)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_removal_batch(CTX(h), (const uint64_t*)m, (const uint32_t*)s, n, &lim, (demi_verdict*)o);
  PUT_LONGS(verdicts, o, 0);
  PUT_INTS(skip, s, JNI_ABORT);
  PUT_LONGS(masksOrNull, m, JNI_ABORT);
  return rc;
}
/* kept: byte[recorded events of the loaded execution] (demi_replay_recorded_len; a shorter array is refused) */
JNIEXPORT jint JNICALL FN(replayGetKept)(JNIEnv* e, jclass c, jlong h, jlongArray maskOrNull, jint skip, jintArray limits,
                                        jlongArray verdict, jbyteArray kept) {
  demi_limits lim;
  demi_verdict v;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(verdict) != 2 || LEN(kept) < 0 || (maskOrNull && LEN(maskOrNull) != 4)) return DEMI_ERR_INVALID_ARG;
  if ((uint64_t)LEN(kept) < (uint64_t)demi_replay_recorded_len(CTX(h))) return DEMI_ERR_CAPACITY;
  memset(&v, 0, sizeof v);
  void* m = LONGS(maskOrNull);
  void* k = BYTES(kept);
  jint rc = (LOST(maskOrNull, m) || LOST(kept, k)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_get_kept(CTX(h), (const uint64_t*)m, (uint32_t)skip, &lim, &v, (uint8_t*)k);
  PUT_BYTES(kept, k, 0);
  PUT_LONGS(maskOrNull, m, JNI_ABORT);
  SET_LONGS(verdict, 2, (const jlong*)(const void*)&v);
  return rc;
}
/* One round of STSSchedMinimizer.minimize (demi_replay_removal_round).  kept: byte[>= recorded events of the loaded execution];
 * result: long[6] = first_hit (-1: none), n_kept, retried, launches, then the winner's verdict as its two words */
JNIEXPORT jint JNICALL FN(replayRemovalRound)(JNIEnv* e, jclass c, jlong h, jlongArray maskOrNull, jintArray skip, jintArray limits,
                                             jbyteArray kept, jlongArray result) {
  demi_limits lim;
  demi_removal_round_result res;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(skip) < 0 || LEN(kept) < 0 || LEN(result) != 6 || (maskOrNull && LEN(maskOrNull) != 4)) return DEMI_ERR_INVALID_ARG;
  if ((uint64_t)LEN(kept) < (uint64_t)demi_replay_recorded_len(CTX(h))) return DEMI_ERR_CAPACITY;
  memset(&res, 0, sizeof res);
  void* m = LONGS(maskOrNull);
  void* s = INTS(skip);
  void* k = BYTES(kept);
  jint rc = (LOST(maskOrNull, m) || LOST(skip, s) || LOST(kept, k)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_removal_round(CTX(h), (const uint64_t*)m, (const uint32_t*)s, (uint32_t)LEN(skip), &lim, (uint8_t*)k, &res);
  PUT_BYTES(kept, k, 0);
  PUT_INTS(skip, s, JNI_ABORT);
  PUT_LONGS(maskOrNull, m, JNI_ABORT);
  jlong r[6];
  r[0] = (jlong)(int32_t)res.first_hit; r[1] = (jlong)res.n_kept; r[2] = (jlong)res.retried; r[3] = (jlong)res.launches;
  memcpy(&r[4], &res.verdict, sizeof res.verdict);
  SET_LONGS(result, 6, r);
  return rc;
}
/* RunnerUtils.minimizeInternals in one call (demi_minimize_internals) on the execution replayLoad loaded; the loaded execution is the
 * minimized one afterwards.  params: int[2] = strategy (0 LeftToRightOneAtATime, 1 SrcDstFIFORemoval), max_batch; trace: byte[16 * cap]
 * receives the minimized recorded events; sizesOrNull: int[] the record_internal_size sequence; stats: long[10] = events of the result,
 * total_replays, replays_run, rounds, launches, adoptions, retried, unignorable, deliveries_before, deliveries_after */
JNIEXPORT jint JNICALL FN(minimizeInternals)(JNIEnv* e, jclass c, jlong h, jintArray limits, jintArray params, jbyteArray trace,
                                            jintArray sizesOrNull, jlongArray stats) {
  demi_limits lim;
  demi_intmin_params par;
  demi_intmin_stats st;
  jint pr[2];
  uint32_t n = 0;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(params) != 2 || LEN(trace) < 0 || LEN(stats) != 10) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 2, pr);
  par.strategy = (uint32_t)pr[0]; par.max_batch = (uint32_t)pr[1];
  memset(&st, 0, sizeof st);
  void* t = BYTES(trace);
  void* z = INTS(sizesOrNull);
  jint rc = (LOST(trace, t) || LOST(sizesOrNull, z)) ? DEMI_ERR_INVALID_ARG
            : demi_minimize_internals(CTX(h), &lim, &par, (demi_rec_event*)t, (uint32_t)(LEN(trace) / (jint)sizeof(demi_rec_event)), &n,
                                      (uint32_t*)z, sizesOrNull ? (uint32_t)LEN(sizesOrNull) : 0u, NULL, 0, &st);
  PUT_INTS(sizesOrNull, z, 0);
  PUT_BYTES(trace, t, 0);
  jlong o[10];
  o[0] = (jlong)n; o[1] = (jlong)st.total_replays; o[2] = (jlong)st.replays_run; o[3] = (jlong)st.rounds; o[4] = (jlong)st.launches;
  o[5] = (jlong)st.adoptions; o[6] = (jlong)st.retried; o[7] = (jlong)st.unignorable; o[8] = (jlong)st.deliveries_before;
  o[9] = (jlong)st.deliveries_after;
  SET_LONGS(stats, 10, o);
  return rc;
}

/* ---- K2W: the replay oracle of the wildcard minimizers (demi_replay_wildcard_*).  typeSets: int[n recorded], policies: byte[n recorded]
 *      (n = demi_replay_recorded_len of the execution replayLoad loaded; shorter arrays are refused) */
JNIEXPORT jint JNICALL FN(replayWildcardLoad)(JNIEnv* e, jclass c, jlong h, jintArray typeSets, jbyteArray policies) {
  (void)c;
  const int64_t n_rec = (int64_t)demi_replay_recorded_len(CTX(h));
  if (!typeSets || !policies || LEN(typeSets) < n_rec || LEN(policies) < n_rec) return DEMI_ERR_INVALID_ARG;
  void* t = INTS(typeSets);
  void* p = BYTES(policies);
  jint rc = (LOST(typeSets, t) || LOST(policies, p)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_wildcard_load(CTX(h), (const uint32_t*)t, (const uint8_t*)p);
  PUT_BYTES(policies, p, JNI_ABORT);
  PUT_INTS(typeSets, t, JNI_ABORT);
  return rc;
}
/* words of one presence row of the loaded execution: ceil(recorded events / 64) */
static int64_t present_words(jlong h) { return ((int64_t)demi_replay_recorded_len(CTX(h)) + 63) / 64; }
/* present: long[words * n] (n from verdicts: long[2 * n]); masksOrNull: long[4 * n] */
JNIEXPORT jint JNICALL FN(replayWildcardBatch)(JNIEnv* e, jclass c, jlong h, jlongArray masksOrNull, jlongArray present, jintArray limits,
                                              jlongArray verdicts) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || !present || LEN(verdicts) < 0 || LEN(verdicts) % 2) return DEMI_ERR_INVALID_ARG;
  const int64_t n = LEN(verdicts) / 2, words = present_words(h);
  if (LEN(present) < words * n || (masksOrNull && LEN(masksOrNull) < 4 * n)) return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masksOrNull);
  void* p = LONGS(present);
  void* o = LONGS(verdicts);
  jint rc = (LOST(masksOrNull, m) || LOST(present, p) || LOST(verdicts, o)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_wildcard_batch(CTX(h), (const uint64_t*)m, (const uint64_t*)p, (uint64_t)n, &lim, (demi_verdict*)o);
  PUT_LONGS(verdicts, o, 0);
  PUT_LONGS(present, p, JNI_ABORT);
  PUT_LONGS(masksOrNull, m, JNI_ABORT);
  return rc;
}
/* maskOrNull: long[4]; present: long[words]; verdict: long[2]; kept: byte[>= recorded events]; recorded: byte[16 * cap];
 * returns the number of events of the executed trace, or a negative demi_status */
JNIEXPORT jint JNICALL FN(replayWildcardGetTrace)(JNIEnv* e, jclass c, jlong h, jlongArray maskOrNull, jlongArray present, jintArray limits,
                                                 jlongArray verdict, jbyteArray kept, jbyteArray recorded) {
  demi_limits lim;
  demi_verdict v;
  (void)c;
  if (limits_of(e, limits, &lim) || !present || LEN(present) < present_words(h) || LEN(verdict) != 2 || LEN(kept) < 0 ||
      (maskOrNull && LEN(maskOrNull) != 4) || LEN(recorded) < 0 || LEN(recorded) % (jint)sizeof(demi_rec_event))
    return DEMI_ERR_INVALID_ARG;
  if ((uint64_t)LEN(kept) < (uint64_t)demi_replay_recorded_len(CTX(h))) return DEMI_ERR_CAPACITY;
  const uint32_t cap = (uint32_t)(LEN(recorded) / (jint)sizeof(demi_rec_event));
  uint32_t n_out = 0;
  memset(&v, 0, sizeof v);
  void* m = LONGS(maskOrNull);
  void* p = LONGS(present);
  void* k = BYTES(kept);
  void* r = BYTES(recorded);
  jint rc = (LOST(maskOrNull, m) || LOST(present, p) || LOST(kept, k) || LOST(recorded, r)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_wildcard_get_trace(CTX(h), (const uint64_t*)m, (const uint64_t*)p, &lim, &v, (uint8_t*)k, (demi_rec_event*)r, cap, &n_out);
  PUT_BYTES(recorded, r, 0);
  PUT_BYTES(kept, k, 0);
  PUT_LONGS(present, p, JNI_ABORT);
  PUT_LONGS(maskOrNull, m, JNI_ABORT);
  SET_LONGS(verdict, 2, (const jlong*)(const void*)&v);
  return rc == DEMI_OK ? (jint)n_out : rc;
}
/* One round of WildcardMinimizer.doMinimize (demi_replay_wildcard_round) over the execution and selectors loaded.  present: long[words * n]
 * (n proposals, each assuming the one before it failed); kept: byte[>= recorded events of the loaded execution]; result: long[8] =
 * first_hit (-1: none), executed_len, n_kept, retried, launches, 0, then the winner's verdict as its two words */
JNIEXPORT jint JNICALL FN(replayWildcardRound)(JNIEnv* e, jclass c, jlong h, jlongArray maskOrNull, jlongArray present, jint n, jintArray limits,
                                              jbyteArray kept, jlongArray result) {
  demi_limits lim;
  demi_wildcard_round_result res;
  (void)c;
  if (limits_of(e, limits, &lim) || !present || n < 0 || LEN(present) < present_words(h) * (int64_t)n || LEN(kept) < 0 || LEN(result) != 8 ||
      (maskOrNull && LEN(maskOrNull) != 4))
    return DEMI_ERR_INVALID_ARG;
  if ((uint64_t)LEN(kept) < (uint64_t)demi_replay_recorded_len(CTX(h))) return DEMI_ERR_CAPACITY;
  memset(&res, 0, sizeof res);
  void* m = LONGS(maskOrNull);
  void* p = LONGS(present);
  void* k = BYTES(kept);
  jint rc = (LOST(maskOrNull, m) || LOST(present, p) || LOST(kept, k)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_wildcard_round(CTX(h), (const uint64_t*)m, (const uint64_t*)p, (uint32_t)n, &lim, (uint8_t*)k, &res);
  PUT_BYTES(kept, k, 0);
  PUT_LONGS(present, p, JNI_ABORT);
  PUT_LONGS(maskOrNull, m, JNI_ABORT);
  jlong r[8];
  r[0] = (jlong)(int32_t)res.first_hit; r[1] = (jlong)res.executed_len; r[2] = (jlong)res.n_kept; r[3] = (jlong)res.retried;
  r[4] = (jlong)res.launches; r[5] = 0;
  memcpy(&r[6], &res.verdict, sizeof res.verdict);
  SET_LONGS(result, 8, r);
  return rc;
}
/* WildcardMinimizer.minimize in one call (demi_minimize_wildcards) on the execution replayLoad loaded; the loaded execution is the minimized
 * one afterwards, without selectors.  params: int[5] = clustering (0 ClockClusterizer, 1 SingletonClusterizer, 2 ClockThenSingleton), policy
 * (0 HEAD, 1 FIRST, 2 LAST), skip_clock_clusters, max_batch, clock_increment_types (bit t); clockField: byte[32] (payload field of the
 * logical clock per message type, -1 = none); trace: byte[16 * cap] receives the minimized recorded events; sizesOrNull: int[] the
 * record_internal_size sequence; stats: long[10] = events of the result, total_replays, replays_run, rounds, launches, adoptions, retried,
 * entries of the sizes sequence, deliveries_before, deliveries_after */
JNIEXPORT jint JNICALL FN(minimizeWildcards)(JNIEnv* e, jclass c, jlong h, jintArray limits, jintArray params, jbyteArray clockField,
                                            jbyteArray trace, jintArray sizesOrNull, jlongArray stats) {
  demi_limits lim;
  demi_wcmin_params par;
  demi_wcmin_stats st;
  jint pr[5];
  uint32_t n = 0;
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(params) != 5 || LEN(clockField) != DEMI_MAX_MSG_TYPES || LEN(trace) < 0 || LEN(stats) != 10)
    return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 5, pr);
  memset(&par, 0, sizeof par);
  par.clustering = (uint32_t)pr[0]; par.policy = (uint32_t)pr[1]; par.skip_clock_clusters = (uint32_t)pr[2]; par.max_batch = (uint32_t)pr[3];
  par.clock_increment_types = (uint32_t)pr[4];
  (*e)->GetByteArrayRegion(e, clockField, 0, DEMI_MAX_MSG_TYPES, (jbyte*)par.clock_field);
  memset(&st, 0, sizeof st);
  void* t = BYTES(trace);
  void* z = INTS(sizesOrNull);
  jint rc = (LOST(trace, t) || LOST(sizesOrNull, z)) ? DEMI_ERR_INVALID_ARG
            : demi_minimize_wildcards(CTX(h), &lim, &par, (demi_rec_event*)t, (uint32_t)(LEN(trace) / (jint)sizeof(demi_rec_event)), &n,
                                      (uint32_t*)z, sizesOrNull ? (uint32_t)LEN(sizesOrNull) : 0u, NULL, 0, &st);
  PUT_INTS(sizesOrNull, z, 0);
  PUT_BYTES(trace, t, 0);
  jlong o[10];
  o[0] = (jlong)n; o[1] = (jlong)st.total_replays; o[2] = (jlong)st.replays_run; o[3] = (jlong)st.rounds; o[4] = (jlong)st.launches;
  o[5] = (jlong)st.adoptions; o[6] = (jlong)st.retried; o[7] = (jlong)st.sizes; o[8] = (jlong)st.deliveries_before;
  o[9] = (jlong)st.deliveries_after;
  SET_LONGS(stats, 10, o);
  return rc;
}
/* ---- WildcardTestOracle.test per candidate (demi_replay_wildcard_candidates).  masks: long[4 * n]; basePresentOrNull: long[words];
 *      drops: int[n_drop] (may be empty); out: long[3 * n] = demi_wildcard_candidate (first_hit | executed_len << 32, flags | first_ovf << 32,
 *      hash); outAllOrNull: long[2 * n * (1 + n_drop)] */
JNIEXPORT jint JNICALL FN(replayWildcardCandidates)(JNIEnv* e, jclass c, jlong h, jlongArray masks, jlongArray basePresentOrNull, jintArray drops,
                                                   jintArray limits, jlongArray out, jlongArray outAllOrNull) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || !masks || LEN(masks) % 4 || !drops || !out) return DEMI_ERR_INVALID_ARG;
  const int64_t n = LEN(masks) / 4, n_drop = LEN(drops);
  if (LEN(out) < 3 * n || (basePresentOrNull && LEN(basePresentOrNull) < present_words(h)) ||
      (outAllOrNull && LEN(outAllOrNull) < 2 * n * (n_drop + 1)))
    return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masks);
  void* b = LONGS(basePresentOrNull);
  void* d = INTS(drops);
  void* o = LONGS(out);
  void* a = LONGS(outAllOrNull);
  jint rc = (LOST(masks, m) || LOST(basePresentOrNull, b) || LOST(drops, d) || LOST(out, o) || LOST(outAllOrNull, a)) ? DEMI_ERR_INVALID_ARG
            : demi_replay_wildcard_candidates(CTX(h), (const uint64_t*)m, (uint32_t)n, (const uint64_t*)b, (const uint32_t*)d, (uint32_t)n_drop,
                                              &lim, (demi_wildcard_candidate*)o, (demi_verdict*)a);
  PUT_LONGS(outAllOrNull, a, 0);
  PUT_LONGS(out, o, 0);
  PUT_INTS(drops, d, JNI_ABORT);
  PUT_LONGS(basePresentOrNull, b, JNI_ABORT);
  PUT_LONGS(masks, m, JNI_ABORT);
  return rc;
}
/* ---- RunnerUtils.wildcardDDMin in one call (demi_wildcard_ddmin).  params, conjoinedOrNull, mcs, consultedOrNull / passedOrNull, stats as
 *      for ddmin; firstHitOrNull: int[cap] (with consultedOrNull; -1 = no proposal reproduced); result: long[13] = total_replays,
 *      proposals_run, mcs_evaluated, mcs_first_hit (-1 = none), mcs_executed_len, mcs_flags, retried, min_first_hit (-1 = none),
 *      min_executed_len, min_externals[4] */
JNIEXPORT jint JNICALL FN(wildcardDDMin)(JNIEnv* e, jclass c, jlong h, jintArray limits, jintArray params, jbyteArray conjoinedOrNull,
                                        jlongArray basePresentOrNull, jintArray drops, jlongArray mcs, jlongArray consultedOrNull,
                                        jbyteArray passedOrNull, jintArray firstHitOrNull, jlongArray stats, jlongArray result) {
  demi_limits lim;
  demi_ddmin_params par;
  demi_ddmin_stats st;
  demi_wildcard_ddmin_result res;
  jint pr[4];
  uint64_t out[4] = {0, 0, 0, 0};
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(params) != 4 || LEN(mcs) != 4 || LEN(stats) != 5 || LEN(result) != 13 || !drops) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 4, pr);
  par.depth = (uint32_t)pr[0]; par.max_candidates = (uint32_t)pr[1]; par.check_unmodified = (uint32_t)pr[2]; par.verify_mcs = (uint32_t)pr[3];
  if (conjoinedOrNull && LEN(conjoinedOrNull) < (int64_t)demi_replay_externals_len(CTX(h))) return DEMI_ERR_INVALID_ARG;
  if (basePresentOrNull && LEN(basePresentOrNull) < present_words(h)) return DEMI_ERR_INVALID_ARG;
  uint32_t cap = 0;
  if (consultedOrNull) {
    if (LEN(consultedOrNull) % 4 || !passedOrNull || LEN(passedOrNull) < LEN(consultedOrNull) / 4 ||
        (firstHitOrNull && LEN(firstHitOrNull) < LEN(consultedOrNull) / 4))
      return DEMI_ERR_INVALID_ARG;
    cap = (uint32_t)(LEN(consultedOrNull) / 4);
  }
  memset(&st, 0, sizeof st);
  memset(&res, 0, sizeof res);
  const int64_t n_drop = LEN(drops);
  void* cj = BYTES(conjoinedOrNull);
  void* bp = LONGS(basePresentOrNull);
  void* dr = INTS(drops);
  void* co = LONGS(consultedOrNull);
  void* pa = BYTES(passedOrNull);
  void* fh = consultedOrNull ? INTS(firstHitOrNull) : NULL;
  jint rc = (LOST(conjoinedOrNull, cj) || LOST(basePresentOrNull, bp) || LOST(drops, dr) || LOST(consultedOrNull, co) || LOST(passedOrNull, pa) ||
             (consultedOrNull && LOST(firstHitOrNull, fh))) ? DEMI_ERR_INVALID_ARG
            : demi_wildcard_ddmin(CTX(h), &lim, &par, (const uint8_t*)cj, (const uint64_t*)bp, (const uint32_t*)dr, (uint32_t)n_drop, out,
                                  (uint64_t*)co, (uint8_t*)pa, (uint32_t*)fh, cap, NULL, 0, &st, &res);
  if (consultedOrNull) PUT_INTS(firstHitOrNull, fh, 0);
  PUT_BYTES(passedOrNull, pa, 0);
  PUT_LONGS(consultedOrNull, co, 0);
  PUT_INTS(drops, dr, JNI_ABORT);
  PUT_LONGS(basePresentOrNull, bp, JNI_ABORT);
  PUT_BYTES(conjoinedOrNull, cj, JNI_ABORT);
  SET_LONGS(mcs, 4, (const jlong*)(const void*)out);
  jlong o[5];
  o[0] = (jlong)st.consultations; o[1] = (jlong)st.launches; o[2] = (jlong)st.mcs_len; o[3] = (jlong)st.verified; o[4] = (jlong)st.replays;
  SET_LONGS(stats, 5, o);
  jlong r[13];
  r[0] = (jlong)res.total_replays; r[1] = (jlong)res.proposals_run; r[2] = (jlong)res.mcs_evaluated; r[3] = (jlong)(int32_t)res.mcs_first_hit;
  r[4] = (jlong)res.mcs_executed_len; r[5] = (jlong)res.mcs_flags; r[6] = (jlong)res.retried;
  r[7] = (jlong)(int32_t)res.min_first_hit; r[8] = (jlong)res.min_executed_len;
  for (int i = 0; i < 4; i++) r[9 + i] = (jlong)res.min_externals[i];
  SET_LONGS(result, 13, r);
  return rc;
}

/* ---- DDMin in one call (demi_ddmin).  params: int[4] (demi_ddmin_params); conjoinedOrNull: byte[>= n externals of replayLoad]; mcs: long[4];
 *      consultedOrNull: long[4 * cap] with passedOrNull: byte[cap]; stats: long[5] = consultations, launches, mcs_len, verified, replays */
JNIEXPORT jint JNICALL FN(ddmin)(JNIEnv* e, jclass c, jlong h, jintArray limits, jintArray params, jbyteArray conjoinedOrNull, jlongArray mcs,
                                jlongArray consultedOrNull, jbyteArray passedOrNull, jlongArray stats) {
  demi_limits lim;
  demi_ddmin_params par;
  demi_ddmin_stats st;
  jint pr[4];
  uint64_t out[4] = {0, 0, 0, 0};
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(params) != 4 || LEN(mcs) != 4 || LEN(stats) != 5) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 4, pr);
  par.depth = (uint32_t)pr[0]; par.max_candidates = (uint32_t)pr[1]; par.check_unmodified = (uint32_t)pr[2]; par.verify_mcs = (uint32_t)pr[3];
  /* demi_ddmin reads conjoined[0 .. n externals of the loaded execution): a shorter array is refused */
  if (conjoinedOrNull && LEN(conjoinedOrNull) < (int64_t)demi_replay_externals_len(CTX(h))) return DEMI_ERR_INVALID_ARG;
  uint32_t cap = 0;
  if (consultedOrNull) {
    if (LEN(consultedOrNull) % 4 || !passedOrNull || LEN(passedOrNull) < LEN(consultedOrNull) / 4) return DEMI_ERR_INVALID_ARG;
    cap = (uint32_t)(LEN(consultedOrNull) / 4);
  }
  memset(&st, 0, sizeof st);
  void* cj = BYTES(conjoinedOrNull);
  void* co = LONGS(consultedOrNull);
  void* pa = BYTES(passedOrNull);
  jint rc = (LOST(conjoinedOrNull, cj) || LOST(consultedOrNull, co) || LOST(passedOrNull, pa)) ? DEMI_ERR_INVALID_ARG
            : demi_ddmin(CTX(h), &lim, &par, (const uint8_t*)cj, out, (uint64_t*)co, (uint8_t*)pa, cap, NULL, 0, &st);
  PUT_BYTES(passedOrNull, pa, 0);
  PUT_LONGS(consultedOrNull, co, 0);
  PUT_BYTES(conjoinedOrNull, cj, JNI_ABORT);
  SET_LONGS(mcs, 4, (const jlong*)(const void*)out);
  jlong o[5];
  o[0] = (jlong)st.consultations; o[1] = (jlong)st.launches; o[2] = (jlong)st.mcs_len; o[3] = (jlong)st.verified; o[4] = (jlong)st.replays;
  SET_LONGS(stats, 5, o);
  return rc;
}

/* ---- RunnerUtils.randomDDMin in one call (demi_random_ddmin) on the externals of traceLoad.  params: int[6] = executions, depth,
 *      max_candidates, check_unmodified, verify_mcs, sequential; conjoinedOrNull: byte[>= n externals]; mcs: long[4]; consultedOrNull:
 *      long[4 * cap] with passedOrNull: byte[cap]; stats: long[5] = consultations, launches, mcs_len, verified, executions run */
JNIEXPORT jint JNICALL FN(randomDDMin)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jintArray limits, jintArray params, jint nExternals,
                                      jbyteArray conjoinedOrNull, jlongArray mcs, jlongArray consultedOrNull, jbyteArray passedOrNull,
                                      jlongArray stats) {
  demi_limits lim;
  demi_random_ddmin_params par;
  demi_ddmin_stats st;
  jint pr[6];
  uint64_t out[4] = {0, 0, 0, 0};
  (void)c;
  if (limits_of(e, limits, &lim) || LEN(params) != 6 || LEN(mcs) != 4 || LEN(stats) != 5 || nExternals < 0) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 6, pr);
  memset(&par, 0, sizeof par);
  par.executions = (uint32_t)pr[0]; par.depth = (uint32_t)pr[1]; par.max_candidates = (uint32_t)pr[2];
  par.check_unmodified = (uint32_t)pr[3]; par.verify_mcs = (uint32_t)pr[4]; par.sequential = (uint32_t)pr[5];
  /* demi_random_ddmin reads conjoined[0 .. n externals of the LOADED trace): the library says how many that is; a caller that
   * states another count, or passes a shorter array, is refused before anything is read */
  if ((uint32_t)nExternals != demi_trace_len(CTX(h))) return DEMI_ERR_INVALID_ARG;
  if (conjoinedOrNull && LEN(conjoinedOrNull) < (int64_t)demi_trace_len(CTX(h))) return DEMI_ERR_INVALID_ARG;
  uint32_t cap = 0;
  if (consultedOrNull) {
    if (LEN(consultedOrNull) % 4 || !passedOrNull || LEN(passedOrNull) < LEN(consultedOrNull) / 4) return DEMI_ERR_INVALID_ARG;
    cap = (uint32_t)(LEN(consultedOrNull) / 4);
  }
  memset(&st, 0, sizeof st);
  void* cj = BYTES(conjoinedOrNull);
  void* co = LONGS(consultedOrNull);
  void* pa = BYTES(passedOrNull);
  jint rc = (LOST(conjoinedOrNull, cj) || LOST(consultedOrNull, co) || LOST(passedOrNull, pa)) ? DEMI_ERR_INVALID_ARG
            : demi_random_ddmin(CTX(h), (uint64_t)seedBase, &lim, &par, (const uint8_t*)cj, out, (uint64_t*)co, (uint8_t*)pa, cap, NULL, 0, &st);
  PUT_BYTES(passedOrNull, pa, 0);
  PUT_LONGS(consultedOrNull, co, 0);
  PUT_BYTES(conjoinedOrNull, cj, JNI_ABORT);
  SET_LONGS(mcs, 4, (const jlong*)(const void*)out);
  jlong o[5];
  o[0] = (jlong)st.consultations; o[1] = (jlong)st.launches; o[2] = (jlong)st.mcs_len; o[3] = (jlong)st.verified; o[4] = (jlong)st.replays;
  SET_LONGS(stats, 5, o);
  return rc;
}

/* ---- RandomScheduler.test for a batch of subsequences of the loaded trace (demi_random_explore_candidates).  masks: long[4 * n];
 *      verdictsOrNull: long[2 * n * executions]; flags: int[n] (bit 0: some execution violates, bit 1: some execution aborted) */
JNIEXPORT jint JNICALL FN(randomExploreCandidates)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jlongArray masks, jint executions,
                                                  jintArray limits, jlongArray verdictsOrNull, jintArray flags) {
  demi_limits lim;
  (void)c;
  const int64_t n = LEN(masks) / 4;
  if (limits_of(e, limits, &lim) || LEN(masks) % 4 || executions <= 0 || !flags || LEN(flags) < n ||
      (verdictsOrNull && LEN(verdictsOrNull) < 2 * n * (int64_t)executions))
    return DEMI_ERR_INVALID_ARG;
  void* m = LONGS(masks);
  void* v = LONGS(verdictsOrNull);
  void* f = INTS(flags);
  jint rc = (LOST(masks, m) || LOST(verdictsOrNull, v) || LOST(flags, f)) ? DEMI_ERR_INVALID_ARG
            : demi_random_explore_candidates(CTX(h), (uint64_t)seedBase, (const uint64_t*)m, (uint32_t)n, (uint32_t)executions, &lim,
                                             (demi_verdict*)v, (uint32_t*)f);
  PUT_INTS(flags, f, 0);
  PUT_LONGS(verdictsOrNull, v, 0);
  PUT_LONGS(masks, m, JNI_ABORT);
  return rc;
}

/* ---- RunnerUtils.editDistanceDporDDMin in one call (demi_edit_distance_dpor_ddmin).  externals: byte[8 * n]; initialTrace: byte[16 * m]
 *      (demi_dpor_trace_entry); dporParams: int[7]; params: int[7] = max_max_distance, stop_at_size, check_unmodified, ignore_quiescence,
 *      verify_mcs, batch, budget; mcs: long[4]; consultedOrNull: long[4 * cap] with passedOrNull: byte[cap] and distanceOrNull: int[cap];
 *      violationTraceOrNull: byte[16 * 256]; stats: long[8 + 32] = replays, interleavings, consultations, instances, passes, mcs_len,
 *      verified, violation_len, pass_distance[16], pass_mcs_len[16] */
JNIEXPORT jint JNICALL FN(editDistanceDporDDMin)(JNIEnv* e, jclass c, jlong h, jbyteArray externals, jbyteArray initialTrace, jintArray dporParams,
                                                jintArray params, jlongArray mcs, jlongArray consultedOrNull, jbyteArray passedOrNull,
                                                jintArray distanceOrNull, jbyteArray violationTraceOrNull, jlongArray stats) {
  demi_dpor_params par;
  demi_incddmin_params ip;
  demi_incddmin_stats st;
  jint pr[7];
  uint64_t out[4] = {0, 0, 0, 0};
  (void)c;
  const int64_t n_ext = LEN(externals), n_init = LEN(initialTrace);
  if (dpor_params_of(e, dporParams, &par) || LEN(params) != 7 || LEN(mcs) != 4 || LEN(stats) != 40 || n_ext < 0 || n_ext % 8 ||
      n_init <= 0 || n_init % (int64_t)sizeof(demi_dpor_trace_entry))
    return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, params, 0, 7, pr);
  memset(&ip, 0, sizeof ip);
  ip.max_max_distance = (uint32_t)pr[0]; ip.stop_at_size = (uint32_t)pr[1]; ip.check_unmodified = (uint32_t)pr[2];
  ip.ignore_quiescence = (uint32_t)pr[3]; ip.verify_mcs = (uint32_t)pr[4]; ip.batch = (uint32_t)pr[5]; ip.budget = (uint32_t)pr[6];
  uint32_t cap = 0;
  if (consultedOrNull) {
    if (LEN(consultedOrNull) % 4 || !passedOrNull || LEN(passedOrNull) < LEN(consultedOrNull) / 4 ||
        (distanceOrNull && LEN(distanceOrNull) < LEN(consultedOrNull) / 4))
      return DEMI_ERR_INVALID_ARG;
    cap = (uint32_t)(LEN(consultedOrNull) / 4);
  }
  if (violationTraceOrNull && LEN(violationTraceOrNull) < (int64_t)sizeof(demi_dpor_trace_entry) * DEMI_DPOR_MAX_TRACE) return DEMI_ERR_INVALID_ARG;
  memset(&st, 0, sizeof st);
  void* ex = BYTES(externals);
  void* it = BYTES(initialTrace);
  void* co = LONGS(consultedOrNull);
  void* pa = BYTES(passedOrNull);
  void* di = consultedOrNull ? INTS(distanceOrNull) : NULL;
  void* vt = BYTES(violationTraceOrNull);
  jint rc = (LOST(externals, ex) || LOST(initialTrace, it) || LOST(consultedOrNull, co) || LOST(passedOrNull, pa) ||
             (consultedOrNull && LOST(distanceOrNull, di)) || LOST(violationTraceOrNull, vt)) ? DEMI_ERR_INVALID_ARG
            : demi_edit_distance_dpor_ddmin(CTX(h), (const demi_ext_event*)ex, (uint32_t)(n_ext / 8), (const demi_dpor_trace_entry*)it,
                                            (uint32_t)(n_init / (int64_t)sizeof(demi_dpor_trace_entry)), &par, &ip, out, (uint64_t*)co,
                                            (uint8_t*)pa, (uint32_t*)di, cap, (demi_dpor_trace_entry*)vt, &st);
  PUT_BYTES(violationTraceOrNull, vt, 0);
  if (consultedOrNull) PUT_INTS(distanceOrNull, di, 0);
  PUT_BYTES(passedOrNull, pa, 0);
  PUT_LONGS(consultedOrNull, co, 0);
  PUT_BYTES(initialTrace, it, JNI_ABORT);
  PUT_BYTES(externals, ex, JNI_ABORT);
  SET_LONGS(mcs, 4, (const jlong*)(const void*)out);
  jlong o[40];
  o[0] = (jlong)st.replays; o[1] = (jlong)st.interleavings; o[2] = (jlong)st.consultations; o[3] = (jlong)st.instances;
  o[4] = (jlong)st.passes; o[5] = (jlong)st.mcs_len; o[6] = (jlong)st.verified; o[7] = (jlong)st.violation_len;
  for (int i = 0; i < 16; i++) { o[8 + i] = (jlong)st.pass_distance[i]; o[24 + i] = (jlong)st.pass_mcs_len[i]; }
  SET_LONGS(stats, 40, o);
  return rc;
}

/* ---- K3 */
JNIEXPORT jint JNICALL FN(dporLoad)(JNIEnv* e, jclass c, jlong h, jbyteArray externals) {
  (void)c;
  const int64_t len = LEN(externals);
  if (len < 0 || len % 8) return DEMI_ERR_INVALID_ARG;
  void* p = BYTES(externals);
  jint rc = LOST(externals, p) ? DEMI_ERR_INVALID_ARG : demi_dpor_load(CTX(h), (const demi_ext_event*)p, (uint32_t)(len / 8));
  PUT_BYTES(externals, p, JNI_ABORT);
  return rc;
}
/* verdicts: long[2 * max_interleavings]; prefixLen, rounds: int[max_interleavings]; firstViolationTrace: byte[16 * 256];
 * stats: long[13] (the demi_dpor_stats fields in order, `fetches` last; the length of the first violating trace is returned, or a negative
 * demi_status).  A whole exploration runs inside this call: no array is pinned critically (see the header). */
JNIEXPORT jint JNICALL FN(dporExplore)(JNIEnv* e, jclass c, jlong h, jintArray params, jintArray search, jlongArray verdicts,
                                      jintArray prefixLen, jintArray rounds, jbyteArray firstViolationTrace, jlongArray stats) {
  demi_dpor_params par;
  demi_dpor_search srch;
  jint s[9];
  (void)c;
  if (dpor_params_of(e, params, &par) || LEN(search) != 9 || LEN(stats) != 13) return DEMI_ERR_INVALID_ARG;
  (*e)->GetIntArrayRegion(e, search, 0, 9, s);
  srch.batch = (uint32_t)s[0]; srch.max_interleavings = (uint32_t)s[1]; srch.stop_if_violation = (uint32_t)s[2];
  srch.track_history = (uint32_t)s[3]; srch.order = (uint32_t)s[4]; srch.cache_mb = (uint32_t)s[5];
  srch.ordering = (uint32_t)s[6]; srch.max_distance_plus1 = (uint32_t)s[7]; srch.resume = (uint32_t)s[8];
  const int64_t cap = (int64_t)srch.max_interleavings;
  if (LEN(verdicts) < 2 * cap || LEN(prefixLen) < cap || (rounds && LEN(rounds) < cap) ||
      (firstViolationTrace && LEN(firstViolationTrace) < (int64_t)sizeof(demi_dpor_trace_entry) * DEMI_DPOR_MAX_TRACE))
    return DEMI_ERR_INVALID_ARG;
  demi_dpor_stats st;
  uint32_t vlen = 0;
  memset(&st, 0, sizeof st);
  void* v = LONGS(verdicts);
  void* pl = INTS(prefixLen);
  void* rd = INTS(rounds);
  void* ft = BYTES(firstViolationTrace);
  jint rc = (LOST(verdicts, v) || LOST(prefixLen, pl) || LOST(rounds, rd) || LOST(firstViolationTrace, ft)) ? DEMI_ERR_INVALID_ARG
            : demi_dpor_explore(CTX(h), &par, &srch, (demi_verdict*)v, (uint32_t*)pl, (uint32_t*)rd, (demi_dpor_trace_entry*)ft, &vlen, &st);
  PUT_BYTES(firstViolationTrace, ft, 0);
  PUT_INTS(rounds, rd, 0);
  PUT_INTS(prefixLen, pl, 0);
  PUT_LONGS(verdicts, v, 0);
  jlong o[13];
  o[0] = (jlong)st.interleavings; o[1] = (jlong)st.launches; o[2] = (jlong)st.violations; o[3] = (jlong)st.first_violation;
  o[4] = (jlong)st.queue_len; o[5] = (jlong)st.exhausted; o[6] = (jlong)st.executed; o[7] = (jlong)st.cache_misses;
  memcpy(&o[8], &st.kernel_ms, sizeof(jlong));
  o[9] = (jlong)st.h2d_bytes; o[10] = (jlong)st.d2h_bytes; o[11] = (jlong)st.backtrack_points; o[12] = (jlong)st.fetches;
  SET_LONGS(stats, 13, o);
  return rc == DEMI_OK ? (jint)vlen : rc;
}

/* ---- demi_dpor_explored: what interleaving `index` of the last dporExplore was.  nextTrace, trace: byte[16 * 256]
 *      (demi_dpor_trace_entry); lens: long[3] = next-trace length, shared length, executed-trace length */
JNIEXPORT jint JNICALL FN(dporExplored)(JNIEnv* e, jclass c, jlong h, jlong index, jbyteArray nextTrace, jbyteArray trace, jlongArray lens) {
  (void)c;
  const int64_t need = (int64_t)sizeof(demi_dpor_trace_entry) * DEMI_DPOR_MAX_TRACE;
  if (index < 0 || !nextTrace || !trace || LEN(nextTrace) < need || LEN(trace) < need || LEN(lens) != 3) return DEMI_ERR_INVALID_ARG;
  uint32_t nl = 0, sl = 0, tl = 0;
  void* nt = BYTES(nextTrace);
  void* tr = BYTES(trace);
  jint rc = (LOST(nextTrace, nt) || LOST(trace, tr)) ? DEMI_ERR_INVALID_ARG
            : demi_dpor_explored(CTX(h), (uint64_t)index, (demi_dpor_trace_entry*)nt, &nl, &sl, (demi_dpor_trace_entry*)tr, &tl);
  PUT_BYTES(trace, tr, 0);
  PUT_BYTES(nextTrace, nt, 0);
  jlong o[3] = {(jlong)nl, (jlong)sl, (jlong)tl};
  SET_LONGS(lens, 3, o);
  return rc;
}

/* ---- demi_dpor_wildcard_batch: n interleavings whose next traces hold wildcards (DPORwHeuristics.scala:474-514), one launch.
 *      prefixes byte[16 * stride * n], prefixLen int[n], params int[7]; outputs: verdicts long[2 * n], traces byte[16 * 256 * n],
 *      traceLen int[n], ignored / wild long[4 * n], alts byte[16 * maxAlts * n] (demi_dpor_wild_alt), nAlts int[n] */
JNIEXPORT jint JNICALL FN(dporWildcardBatch)(JNIEnv* e, jclass c, jlong h, jbyteArray prefixes, jintArray prefixLen, jint stride, jintArray params,
                                             jboolean stopAfterNextTrace, jint maxAlts, jlongArray verdicts, jbyteArray traces, jintArray traceLen,
                                             jlongArray ignored, jlongArray wild, jbyteArray alts, jintArray nAlts) {
  (void)c;
  demi_dpor_params par;
  const int64_t n = LEN(prefixLen), esz = (int64_t)sizeof(demi_dpor_trace_entry);
  if (dpor_params_of(e, params, &par) || n <= 0 || stride < 0 || stride > 256 || maxAlts < 0 || maxAlts > 256 ||
      LEN(prefixes) < esz * stride * n || LEN(verdicts) < 2 * n || LEN(traces) < esz * DEMI_DPOR_MAX_TRACE * n || LEN(traceLen) < n ||
      LEN(ignored) < 4 * n || LEN(wild) < 4 * n || (maxAlts && LEN(alts) < (int64_t)sizeof(demi_dpor_wild_alt) * maxAlts * n) || LEN(nAlts) < n)
    return DEMI_ERR_INVALID_ARG;
  void* pf = BYTES(prefixes); void* pl = INTS(prefixLen); void* v = LONGS(verdicts); void* tr = BYTES(traces); void* tl = INTS(traceLen);
  void* ig = LONGS(ignored); void* wc = LONGS(wild); void* al = maxAlts ? BYTES(alts) : NULL; void* na = INTS(nAlts);
  jint rc = (LOST(prefixes, pf) || LOST(prefixLen, pl) || LOST(verdicts, v) || LOST(traces, tr) || LOST(traceLen, tl) || LOST(ignored, ig) ||
             LOST(wild, wc) || (maxAlts && LOST(alts, al)) || LOST(nAlts, na))
                ? DEMI_ERR_INVALID_ARG
                : demi_dpor_wildcard_batch(CTX(h), (const demi_dpor_trace_entry*)pf, (const uint32_t*)pl, (uint32_t)stride, (uint64_t)n, &par,
                                           stopAfterNextTrace ? 1u : 0u, (uint32_t)maxAlts, (demi_verdict*)v, (demi_dpor_trace_entry*)tr,
                                           (uint32_t*)tl, (uint64_t*)ig, (uint64_t*)wc, (demi_dpor_wild_alt*)al, (uint32_t*)na);
  PUT_INTS(nAlts, na, 0); if (maxAlts) PUT_BYTES(alts, al, 0); PUT_LONGS(wild, wc, 0); PUT_LONGS(ignored, ig, 0); PUT_INTS(traceLen, tl, 0);
  PUT_BYTES(traces, tr, 0); PUT_LONGS(verdicts, v, 0); PUT_INTS(prefixLen, pl, JNI_ABORT); PUT_BYTES(prefixes, pf, JNI_ABORT);
  return rc;
}

/* ---- WildcardMinimizer.testWithDpor of one proposal (demi_wildcard_dpor_test, WildcardMinimizer.scala:67-114).  initial byte[16 * m]
 *      (kind 3 / 4 entries); params int[7]; wc int[3] = dpor_budget, batch, max_alts; trace byte[16 * 256]; result long[16] =
 *      hit, interleavings, speculated, launches, exhausted, budget_reached, retried, trace_len, skipped_explored, points, 0, 0,
 *      ignored[0 .. 3] */
JNIEXPORT jint JNICALL FN(wildcardDporTest)(JNIEnv* e, jclass c, jlong h, jbyteArray initial, jintArray params, jintArray wc, jbyteArray trace,
                                            jlongArray result) {
  (void)c;
  demi_dpor_params par;
  const int64_t n_init = LEN(initial), esz = (int64_t)sizeof(demi_dpor_trace_entry);
  if (dpor_params_of(e, params, &par) || LEN(wc) != 3 || n_init < 0 || n_init % esz || !trace || LEN(trace) < esz * DEMI_DPOR_MAX_TRACE ||
      LEN(result) != 16)
    return DEMI_ERR_INVALID_ARG;
  jint w[3];
  (*e)->GetIntArrayRegion(e, wc, 0, 3, w);
  demi_wcdpor_params wp = {(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], 0};
  demi_wcdpor_result r;
  memset(&r, 0, sizeof r);
  void* it = BYTES(initial);
  void* tr = BYTES(trace);
  jint rc = (LOST(initial, it) || LOST(trace, tr)) ? DEMI_ERR_INVALID_ARG
            : demi_wildcard_dpor_test(CTX(h), (const demi_dpor_trace_entry*)it, (uint32_t)(n_init / esz), &par, &wp, (demi_dpor_trace_entry*)tr, &r);
  PUT_BYTES(trace, tr, 0);
  PUT_BYTES(initial, it, JNI_ABORT);
  jlong o[16] = {(jlong)r.hit, (jlong)r.interleavings, (jlong)r.speculated, (jlong)r.launches, (jlong)r.exhausted, (jlong)r.budget_reached,
                 (jlong)r.retried, (jlong)r.trace_len, (jlong)r.skipped_explored, (jlong)r.points, 0, 0,
                 (jlong)r.ignored[0], (jlong)r.ignored[1], (jlong)r.ignored[2], (jlong)r.ignored[3]};
  SET_LONGS(result, 16, o);
  return rc;
}

/* ---- ProvenanceTracker.pruneConcurrentEvents for a batch of traces: traces byte[16 * stride * n] (demi_dpor_trace_entry),
 *      traceLen int[n], affected int[n] (actor bitmasks), keep long[4 * n] */
JNIEXPORT jint JNICALL FN(provenancePrune)(JNIEnv* e, jclass c, jlong h, jbyteArray traces, jintArray traceLen, jintArray affected,
                                          jint stride, jlongArray keep) {
  (void)c;
  const int64_t n = LEN(traceLen);
  if (n < 0 || stride < 0 || LEN(affected) < n || LEN(keep) < 4 * n ||
      LEN(traces) < (int64_t)sizeof(demi_dpor_trace_entry) * (int64_t)stride * n)
    return DEMI_ERR_INVALID_ARG;
  void* t = BYTES(traces);
  void* l = INTS(traceLen);
  void* a = INTS(affected);
  void* k = LONGS(keep);
  jint rc = (LOST(traces, t) || LOST(traceLen, l) || LOST(affected, a) || LOST(keep, k)) ? DEMI_ERR_INVALID_ARG
            : demi_provenance_prune(CTX(h), (const demi_dpor_trace_entry*)t, (const uint32_t*)l, (const uint32_t*)a, (uint32_t)stride,
                                    (uint64_t)n, (uint64_t*)k);
  PUT_LONGS(keep, k, 0);
  PUT_INTS(affected, a, JNI_ABORT);
  PUT_INTS(traceLen, l, JNI_ABORT);
  PUT_BYTES(traces, t, JNI_ABORT);
  return rc;
}

/* ArvindDistanceOrdering.init / setInitialTrace for the following dporExplore calls: originalKeys long[n] (node keys) or null,
 * initialTrace byte[16 * m] (demi_dpor_trace_entry) or null */
JNIEXPORT jint JNICALL FN(dporSetTraces)(JNIEnv* e, jclass c, jlong h, jlongArray originalKeysOrNull, jbyteArray initialTraceOrNull) {
  (void)c;
  const int64_t lk = originalKeysOrNull ? LEN(originalKeysOrNull) : 0, lt = initialTraceOrNull ? LEN(initialTraceOrNull) : 0;
  if (lk < 0 || lt < 0 || lt % (int64_t)sizeof(demi_dpor_trace_entry)) return DEMI_ERR_INVALID_ARG;
  void* k = LONGS(originalKeysOrNull);
  void* t = BYTES(initialTraceOrNull);
  jint rc = (LOST(originalKeysOrNull, k) || LOST(initialTraceOrNull, t)) ? DEMI_ERR_INVALID_ARG
            : demi_dpor_set_traces(CTX(h), (const uint64_t*)k, (uint32_t)lk, (const demi_dpor_trace_entry*)t,
                                   (uint32_t)(lt / (int64_t)sizeof(demi_dpor_trace_entry)));
  PUT_BYTES(initialTraceOrNull, t, JNI_ABORT);
  PUT_LONGS(originalKeysOrNull, k, JNI_ABORT);
  return rc;
}

/* ---- multi-GPU: one JVM (and one ctx) per GPU; rank 0 obtains the id and sends the 128 bytes to the others */
JNIEXPORT jint JNICALL FN(commUniqueId)(JNIEnv* e, jclass c, jbyteArray id128) {
  demi_comm_id id;
  (void)c;
  if (LEN(id128) != (int64_t)sizeof id) return DEMI_ERR_INVALID_ARG;
  jint rc = demi_comm_unique_id(&id);
  if (rc == DEMI_OK) (*e)->SetByteArrayRegion(e, id128, 0, (jsize)sizeof id, (const jbyte*)(const void*)&id);
  return rc;
}
JNIEXPORT jint JNICALL FN(commCreate)(JNIEnv* e, jclass c, jlong h, jbyteArray id128, jint rank, jint world) {
  demi_comm_id id;
  (void)c;
  if (LEN(id128) != (int64_t)sizeof id) return DEMI_ERR_INVALID_ARG;
  (*e)->GetByteArrayRegion(e, id128, 0, (jsize)sizeof id, (jbyte*)(void*)&id);
  return demi_comm_create(CTX(h), &id, rank, world);
}
JNIEXPORT jint JNICALL FN(commDestroy)(JNIEnv* e, jclass c, jlong h) { (void)e; (void)c; return demi_comm_destroy(CTX(h)); }
/* out: long[2 * cap] merged violation set; count: long[1] */
JNIEXPORT jint JNICALL FN(randomExploreSharded)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jlong nTotal, jintArray limits,
                                               jlongArray out, jlongArray count) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || nTotal < 0 || LEN(out) < 0 || LEN(out) % 2 || LEN(count) != 1) return DEMI_ERR_INVALID_ARG;
  const uint32_t cap = (uint32_t)(LEN(out) / 2);
  uint64_t n = 0;
  void* o = LONGS(out);
  jint rc = LOST(out, o) ? DEMI_ERR_INVALID_ARG
                         : demi_random_explore_sharded(CTX(h), (uint64_t)seedBase, (uint64_t)nTotal, &lim, (demi_violation*)o, cap, &n);
  PUT_LONGS(out, o, 0);
  const jlong cn = (jlong)n;
  SET_LONGS(count, 1, &cn);
  return rc;
}

/* ---- fuzz campaigns (demi_fuzz_generate / demi_random_explore_tests / demi_fuzz_campaign).  A Fuzzer crosses as: numEvents; prefix,
 *      postfixOrNull: byte[8 * n] (demi_ext_event); weightBits: long[5] = Double.doubleToRawLongBits of total_mass, cum[0 .. 3] (summed by
 *      the caller in FuzzerWeights' own order); gen: byte[136] (demi_fuzz_send_gen).  The arrays are copied: nothing of them is pinned
 *      while the device works. */
typedef struct { demi_fuzz_params par; demi_ext_event fix[2 * DEMI_MAX_EXT_EVENTS]; } jni_fuzzer;
static int fuzzer_of(JNIEnv* e, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull, jlongArray weightBits, jbyteArray gen, jni_fuzzer* f) {
  const int64_t np = LEN(prefix), nq = postfixOrNull ? LEN(postfixOrNull) : 0;
  jlong w[5];
  memset(f, 0, sizeof *f);
  if (numEvents < 0 || np < 0 || np % 8 || nq % 8 || np / 8 > DEMI_MAX_EXT_EVENTS || nq / 8 > DEMI_MAX_EXT_EVENTS || LEN(weightBits) != 5 ||
      (gen && LEN(gen) != (int64_t)sizeof(demi_fuzz_send_gen)))      /* (gen = NULL: the *Fields entry points, whose generator travels beside) */
    return DEMI_ERR_INVALID_ARG;
  (*e)->GetByteArrayRegion(e, prefix, 0, (jsize)np, (jbyte*)f->fix);
  if (nq) (*e)->GetByteArrayRegion(e, postfixOrNull, 0, (jsize)nq, (jbyte*)(f->fix + DEMI_MAX_EXT_EVENTS));
  if (gen) (*e)->GetByteArrayRegion(e, gen, 0, (jsize)sizeof(demi_fuzz_send_gen), (jbyte*)&f->par.gen);
  {
    void* wb = LONGS(weightBits);
    if (LOST(weightBits, wb)) return DEMI_ERR_INVALID_ARG;
    memcpy(w, wb, sizeof w);
    PUT_LONGS(weightBits, wb, JNI_ABORT);
  }
  memcpy(&f->par.total_mass, &w[0], sizeof(double));
  memcpy(f->par.cum, &w[1], 4 * sizeof(double));
  f->par.num_events = (uint32_t)numEvents; f->par.n_prefix = (uint32_t)(np / 8); f->par.n_postfix = (uint32_t)(nq / 8);
  f->par.prefix = f->fix; f->par.postfix = nq ? f->fix + DEMI_MAX_EXT_EVENTS : NULL;
  return DEMI_OK;
}

/* eventsOrNull: byte[8 * nTests * stride] with stride = prefix + numEvents + postfix + 1 events; nEv: int[nTests]; nBatchesOrNull: int[nTests];
 * seedsOrNull: long[nTests] */
JNIEXPORT jint JNICALL FN(fuzzGenerate)(JNIEnv* e, jclass c, jlong h, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull,
                                       jlongArray weightBits, jbyteArray gen, jlong seedBase, jlongArray seedsOrNull, jint nTests,
                                       jbyteArray eventsOrNull, jintArray nEv, jintArray nBatchesOrNull) {
  jni_fuzzer f;
  (void)c;
  if (fuzzer_of(e, numEvents, prefix, postfixOrNull, weightBits, gen, &f) || nTests < 0 || !nEv || LEN(nEv) < nTests ||
      (nBatchesOrNull && LEN(nBatchesOrNull) < nTests) || (seedsOrNull && LEN(seedsOrNull) < nTests) ||
      (eventsOrNull && LEN(eventsOrNull) < 8 * (int64_t)nTests * (int64_t)demi_fuzz_stride(&f.par)))
    return DEMI_ERR_INVALID_ARG;
  void* sd = LONGS(seedsOrNull);
  void* ev = BYTES(eventsOrNull);
  void* ne = INTS(nEv);
  void* nb = INTS(nBatchesOrNull);
  jint rc = (LOST(seedsOrNull, sd) || LOST(eventsOrNull, ev) || LOST(nEv, ne) || LOST(nBatchesOrNull, nb)) ? DEMI_ERR_INVALID_ARG
            : demi_fuzz_generate(CTX(h), &f.par, (uint64_t)seedBase, (const uint64_t*)sd, (uint32_t)nTests, (demi_ext_event*)ev, (uint32_t*)ne,
                                 (uint32_t*)nb);
  PUT_INTS(nBatchesOrNull, nb, 0);
  PUT_INTS(nEv, ne, 0);
  PUT_BYTES(eventsOrNull, ev, 0);
  PUT_LONGS(seedsOrNull, sd, JNI_ABORT);
  return rc;
}

/* testsOrNull: byte[8 * nTests * stride] with nEvOrNull: int[nTests], or null for the tests fuzzGenerate left in the context;
 * verdictsOrNull: long[2 * nTests * executions]; flags: int[nTests] (bit 0: some execution violates, bit 1: some execution aborted) */
JNIEXPORT jint JNICALL FN(randomExploreTests)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jbyteArray testsOrNull, jintArray nEvOrNull,
                                             jint stride, jint nTests, jint executions, jintArray limits, jlongArray verdictsOrNull,
                                             jintArray flags) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || nTests < 0 || executions < 0 || stride < 0 || !flags || LEN(flags) < nTests ||
      (verdictsOrNull && LEN(verdictsOrNull) < 2 * (int64_t)nTests * (int64_t)executions) ||
      (testsOrNull && (!nEvOrNull || LEN(nEvOrNull) < nTests || LEN(testsOrNull) < 8 * (int64_t)nTests * (int64_t)stride)))
    return DEMI_ERR_INVALID_ARG;
  void* t = BYTES(testsOrNull);
  void* ne = testsOrNull ? INTS(nEvOrNull) : NULL;
  void* v = LONGS(verdictsOrNull);
  void* fl = INTS(flags);
  jint rc = (LOST(testsOrNull, t) || (testsOrNull && LOST(nEvOrNull, ne)) || LOST(verdictsOrNull, v) || LOST(flags, fl)) ? DEMI_ERR_INVALID_ARG
            : demi_random_explore_tests(CTX(h), (uint64_t)seedBase, (const demi_ext_event*)t, (const uint32_t*)ne, (uint32_t)stride,
                                        (uint32_t)nTests, (uint32_t)executions, &lim, (demi_verdict*)v, (uint32_t*)fl);
  PUT_INTS(flags, fl, 0);
  PUT_LONGS(verdictsOrNull, v, 0);
  if (testsOrNull) PUT_INTS(nEvOrNull, ne, JNI_ABORT);
  PUT_BYTES(testsOrNull, t, JNI_ABORT);
  return rc;
}

/* campaign: long[5] = test_seed_base, exec_seed_base, executions_per_test, tests_per_launch, max_tests; events: byte[8 * 255] (the
 * violating test); result: long[9] = found, test_index, exec_index, n_events, tests_run, launches, capacity_aborts, the verdict's
 * flags | fingerprint << 32, its hash */
JNIEXPORT jint JNICALL FN(fuzzCampaign)(JNIEnv* e, jclass c, jlong h, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull,
                                       jlongArray weightBits, jbyteArray gen, jlongArray campaign, jintArray limits, jbyteArray events,
                                       jlongArray result) {
  jni_fuzzer f;
  demi_limits lim;
  demi_fuzz_campaign_params cp;
  demi_fuzz_campaign_result res;
  jlong o[9];
  (void)c;
  if (fuzzer_of(e, numEvents, prefix, postfixOrNull, weightBits, gen, &f) || limits_of(e, limits, &lim) || LEN(campaign) != 5 ||
      LEN(result) != 9 || !events || LEN(events) < 8 * DEMI_MAX_EXT_EVENTS)
    return DEMI_ERR_INVALID_ARG;
  memset(&cp, 0, sizeof cp);
  {
    void* cb = LONGS(campaign);
    if (LOST(campaign, cb)) return DEMI_ERR_INVALID_ARG;
    const jlong* q = (const jlong*)cb;
    cp.test_seed_base = (uint64_t)q[0]; cp.exec_seed_base = (uint64_t)q[1]; cp.executions_per_test = (uint32_t)q[2];
    cp.tests_per_launch = (uint32_t)q[3]; cp.max_tests = (uint32_t)q[4];
    PUT_LONGS(campaign, cb, JNI_ABORT);
  }
  void* ev = BYTES(events);
  jint rc = LOST(events, ev) ? DEMI_ERR_INVALID_ARG
            : demi_fuzz_campaign(CTX(h), &f.par, &cp, &lim, (demi_ext_event*)ev, DEMI_MAX_EXT_EVENTS, &res);
  PUT_BYTES(events, ev, 0);
  if (rc) return rc;
  o[0] = (jlong)res.found; o[1] = (jlong)res.test_index; o[2] = (jlong)res.exec_index; o[3] = (jlong)res.n_events; o[4] = (jlong)res.tests_run;
  o[5] = (jlong)res.launches; o[6] = (jlong)res.capacity_aborts;
  o[7] = (jlong)((uint64_t)res.verdict.flags | ((uint64_t)res.verdict.fingerprint << 32)); o[8] = (jlong)res.verdict.hash;
  SET_LONGS(result, 9, o);
  return rc;
}

/* ---- the same for messages with more than two fields (demi_fuzz_generate_fields / demi_random_explore_tests_areas /
 *      demi_fuzz_campaign_fields): fieldGen: byte[296] (demi_fuzz_field_gen); areas: long[] beside every byte[8 * ..] of events */
static int field_gen_of(JNIEnv* e, jbyteArray fieldGen, demi_fuzz_field_gen* g) {
  if (!fieldGen || LEN(fieldGen) != (int64_t)sizeof(demi_fuzz_field_gen)) return DEMI_ERR_INVALID_ARG;
  (*e)->GetByteArrayRegion(e, fieldGen, 0, (jsize)sizeof(demi_fuzz_field_gen), (jbyte*)g);
  return DEMI_OK;
}

/* areasOrNull: long[nTests * stride], beside eventsOrNull */
JNIEXPORT jint JNICALL FN(fuzzGenerateFields)(JNIEnv* e, jclass c, jlong h, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull,
                                             jlongArray weightBits, jbyteArray fieldGen, jlong seedBase, jlongArray seedsOrNull, jint nTests,
                                             jbyteArray eventsOrNull, jlongArray areasOrNull, jintArray nEv, jintArray nBatchesOrNull) {
  jni_fuzzer f;
  demi_fuzz_field_gen g;
  (void)c;
  if (fuzzer_of(e, numEvents, prefix, postfixOrNull, weightBits, NULL, &f) || field_gen_of(e, fieldGen, &g) || nTests < 0 || !nEv ||
      LEN(nEv) < nTests || (nBatchesOrNull && LEN(nBatchesOrNull) < nTests) || (seedsOrNull && LEN(seedsOrNull) < nTests) ||
      (eventsOrNull && LEN(eventsOrNull) < 8 * (int64_t)nTests * (int64_t)demi_fuzz_stride(&f.par)) ||
      (areasOrNull && LEN(areasOrNull) < (int64_t)nTests * (int64_t)demi_fuzz_stride(&f.par)))
    return DEMI_ERR_INVALID_ARG;
  void* sd = LONGS(seedsOrNull);
  void* ev = BYTES(eventsOrNull);
  void* ar = LONGS(areasOrNull);
  void* ne = INTS(nEv);
  void* nb = INTS(nBatchesOrNull);
  jint rc = (LOST(seedsOrNull, sd) || LOST(eventsOrNull, ev) || LOST(areasOrNull, ar) || LOST(nEv, ne) || LOST(nBatchesOrNull, nb))
                ? DEMI_ERR_INVALID_ARG
                : demi_fuzz_generate_fields(CTX(h), &f.par, &g, (uint64_t)seedBase, (const uint64_t*)sd, (uint32_t)nTests, (demi_ext_event*)ev,
                                            (uint64_t*)ar, (uint32_t*)ne, (uint32_t*)nb);
  PUT_INTS(nBatchesOrNull, nb, 0);
  PUT_INTS(nEv, ne, 0);
  PUT_LONGS(areasOrNull, ar, 0);
  PUT_BYTES(eventsOrNull, ev, 0);
  PUT_LONGS(seedsOrNull, sd, JNI_ABORT);
  return rc;
}

/* randomExploreTests for any table: areasOrNull: long[nTests * stride] beside testsOrNull (null with tests: the areas are made of
 * P0 / P1; testsOrNull = null: the events and areas fuzzGenerateFields left in the context) */
JNIEXPORT jint JNICALL FN(randomExploreTestsAreas)(JNIEnv* e, jclass c, jlong h, jlong seedBase, jbyteArray testsOrNull, jlongArray areasOrNull,
                                                  jintArray nEvOrNull, jint stride, jint nTests, jint executions, jintArray limits,
                                                  jlongArray verdictsOrNull, jintArray flags) {
  demi_limits lim;
  (void)c;
  if (limits_of(e, limits, &lim) || nTests < 0 || executions < 0 || stride < 0 || !flags || LEN(flags) < nTests ||
      (verdictsOrNull && LEN(verdictsOrNull) < 2 * (int64_t)nTests * (int64_t)executions) ||
      (testsOrNull && (!nEvOrNull || LEN(nEvOrNull) < nTests || LEN(testsOrNull) < 8 * (int64_t)nTests * (int64_t)stride)) ||
      (areasOrNull && (!testsOrNull || LEN(areasOrNull) < (int64_t)nTests * (int64_t)stride)))
    return DEMI_ERR_INVALID_ARG;
  void* t = BYTES(testsOrNull);
  void* ar = LONGS(areasOrNull);
  void* ne = testsOrNull ? INTS(nEvOrNull) : NULL;
  void* v = LONGS(verdictsOrNull);
  void* fl = INTS(flags);
  jint rc = (LOST(testsOrNull, t) || LOST(areasOrNull, ar) || (testsOrNull && LOST(nEvOrNull, ne)) || LOST(verdictsOrNull, v) || LOST(flags, fl))
                ? DEMI_ERR_INVALID_ARG
                : demi_random_explore_tests_areas(CTX(h), (uint64_t)seedBase, (const demi_ext_event*)t, (const uint64_t*)ar, (const uint32_t*)ne,
                                                  (uint32_t)stride, (uint32_t)nTests, (uint32_t)executions, &lim, (demi_verdict*)v, (uint32_t*)fl);
  PUT_INTS(flags, fl, 0);
  PUT_LONGS(verdictsOrNull, v, 0);
  if (testsOrNull) PUT_INTS(nEvOrNull, ne, JNI_ABORT);
  PUT_LONGS(areasOrNull, ar, JNI_ABORT);
  PUT_BYTES(testsOrNull, t, JNI_ABORT);
  return rc;
}

/* fuzzCampaign with fieldGen; areas: long[255] (the violating test's payload areas) */
JNIEXPORT jint JNICALL FN(fuzzCampaignFields)(JNIEnv* e, jclass c, jlong h, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull,
                                             jlongArray weightBits, jbyteArray fieldGen, jlongArray campaign, jintArray limits,
                                             jbyteArray events, jlongArray areas, jlongArray result) {
  jni_fuzzer f;
  demi_fuzz_field_gen g;
  demi_limits lim;
  demi_fuzz_campaign_params cp;
  demi_fuzz_campaign_result res;
  jlong o[9];
  (void)c;
  if (fuzzer_of(e, numEvents, prefix, postfixOrNull, weightBits, NULL, &f) || field_gen_of(e, fieldGen, &g) || limits_of(e, limits, &lim) ||
      LEN(campaign) != 5 || LEN(result) != 9 || !events || LEN(events) < 8 * DEMI_MAX_EXT_EVENTS || !areas || LEN(areas) < DEMI_MAX_EXT_EVENTS)
    return DEMI_ERR_INVALID_ARG;
  memset(&cp, 0, sizeof cp);
  {
    void* cb = LONGS(campaign);
    if (LOST(campaign, cb)) return DEMI_ERR_INVALID_ARG;
    const jlong* q = (const jlong*)cb;
    cp.test_seed_base = (uint64_t)q[0]; cp.exec_seed_base = (uint64_t)q[1]; cp.executions_per_test = (uint32_t)q[2];
    cp.tests_per_launch = (uint32_t)q[3]; cp.max_tests = (uint32_t)q[4];
    PUT_LONGS(campaign, cb, JNI_ABORT);
  }
  void* ev = BYTES(events);
  void* ar = LONGS(areas);
  jint rc = (LOST(events, ev) || LOST(areas, ar)) ? DEMI_ERR_INVALID_ARG
            : demi_fuzz_campaign_fields(CTX(h), &f.par, &g, &cp, &lim, (demi_ext_event*)ev, (uint64_t*)ar, DEMI_MAX_EXT_EVENTS, &res);
  PUT_LONGS(areas, ar, 0);
  PUT_BYTES(events, ev, 0);
  if (rc) return rc;
  o[0] = (jlong)res.found; o[1] = (jlong)res.test_index; o[2] = (jlong)res.exec_index; o[3] = (jlong)res.n_events; o[4] = (jlong)res.tests_run;
  o[5] = (jlong)res.launches; o[6] = (jlong)res.capacity_aborts;
  o[7] = (jlong)((uint64_t)res.verdict.flags | ((uint64_t)res.verdict.fingerprint << 32)); o[8] = (jlong)res.verdict.hash;
  SET_LONGS(result, 9, o);
  return rc;
}

/* ---- a launch reduced on the device, campaigns with launches in flight (demi_fuzz_launch_summary / _row, demi_fuzz_campaign_pipelined) */
/* flagsOrNull: int[nTests] with verdictsOrNull: long[2 * nTests * executions], or both null (the resident results); result: long[8] =
 * first_hit, capacity_aborts, exec_index, aborted_before, n_events, 0, the verdict's flags | fingerprint << 32, its hash; eventsOrNull:
 * byte[8 * 255], areasOrNull: long[255] (the violating test of the resident form) */
JNIEXPORT jint JNICALL FN(fuzzLaunchSummary)(JNIEnv* e, jclass c, jlong h, jintArray flagsOrNull, jlongArray verdictsOrNull, jint nTests,
                                            jint executions, jbyteArray eventsOrNull, jlongArray areasOrNull, jlongArray result) {
  demi_fuzz_summary s;
  jlong o[8];
  (void)c;
  if (nTests < 0 || executions < 0 || LEN(result) != 8 || (flagsOrNull == NULL) != (verdictsOrNull == NULL) ||
      (flagsOrNull && (LEN(flagsOrNull) < nTests || LEN(verdictsOrNull) < 2 * (int64_t)nTests * (int64_t)executions)) ||
      (eventsOrNull && LEN(eventsOrNull) < 8 * DEMI_MAX_EXT_EVENTS) || (areasOrNull && (!eventsOrNull || LEN(areasOrNull) < DEMI_MAX_EXT_EVENTS)))
    return DEMI_ERR_INVALID_ARG;
  void* fl = INTS(flagsOrNull);
  void* v = LONGS(verdictsOrNull);
  jint rc = (LOST(flagsOrNull, fl) || LOST(verdictsOrNull, v)) ? DEMI_ERR_INVALID_ARG
            : demi_fuzz_launch_summary(CTX(h), (const uint32_t*)fl, (const demi_verdict*)v, (uint32_t)nTests, (uint32_t)executions, &s);
  PUT_LONGS(verdictsOrNull, v, JNI_ABORT);
  PUT_INTS(flagsOrNull, fl, JNI_ABORT);
  if (rc) return rc;
  if (eventsOrNull && !flagsOrNull) {
    void* ev = BYTES(eventsOrNull);
    void* ar = LONGS(areasOrNull);
    rc = (LOST(eventsOrNull, ev) || LOST(areasOrNull, ar)) ? DEMI_ERR_INVALID_ARG
         : demi_fuzz_launch_summary_row(CTX(h), (demi_ext_event*)ev, (uint64_t*)ar, DEMI_MAX_EXT_EVENTS);
    PUT_LONGS(areasOrNull, ar, 0);
    PUT_BYTES(eventsOrNull, ev, 0);
    if (rc) return rc;
  }
  o[0] = (jlong)s.first_hit; o[1] = (jlong)s.capacity_aborts; o[2] = (jlong)s.exec_index; o[3] = (jlong)s.aborted_before; o[4] = (jlong)s.n_events;
  o[5] = 0; o[6] = (jlong)((uint64_t)s.verdict.flags | ((uint64_t)s.verdict.fingerprint << 32)); o[7] = (jlong)s.verdict.hash;
  SET_LONGS(result, 8, o);
  return rc;
}

/* fuzzCampaign (genOrNull: byte[136]) or fuzzCampaignFields (fieldGenOrNull: byte[296], areasOrNull: long[255]) - exactly one generator -
 * with inFlight launches on the device at a time; statsOrNull: long[2] = launches_submitted, launches_discarded */
JNIEXPORT jint JNICALL FN(fuzzCampaignPipelined)(JNIEnv* e, jclass c, jlong h, jint numEvents, jbyteArray prefix, jbyteArray postfixOrNull,
                                                jlongArray weightBits, jbyteArray genOrNull, jbyteArray fieldGenOrNull, jlongArray campaign,
                                                jint inFlight, jintArray limits, jbyteArray events, jlongArray areasOrNull, jlongArray result,
                                                jlongArray statsOrNull) {
  jni_fuzzer f;
  demi_fuzz_field_gen g;
  demi_limits lim;
  demi_fuzz_campaign_params cp;
  demi_fuzz_pipeline_params pp;
  demi_fuzz_campaign_result res;
  demi_fuzz_pipeline_stats st;
  jlong o[9], so[2];
  (void)c;
  if ((genOrNull == NULL) == (fieldGenOrNull == NULL) || inFlight < 0 || fuzzer_of(e, numEvents, prefix, postfixOrNull, weightBits, genOrNull, &f) ||
      (fieldGenOrNull && field_gen_of(e, fieldGenOrNull, &g)) || limits_of(e, limits, &lim) || LEN(campaign) != 5 || LEN(result) != 9 || !events ||
      LEN(events) < 8 * DEMI_MAX_EXT_EVENTS || (areasOrNull && LEN(areasOrNull) < DEMI_MAX_EXT_EVENTS) || (statsOrNull && LEN(statsOrNull) != 2))
    return DEMI_ERR_INVALID_ARG;
  memset(&cp, 0, sizeof cp);
  memset(&pp, 0, sizeof pp);
  pp.in_flight = (uint32_t)inFlight;
  {
    void* cb = LONGS(campaign);
    if (LOST(campaign, cb)) return DEMI_ERR_INVALID_ARG;
    const jlong* q = (const jlong*)cb;
    cp.test_seed_base = (uint64_t)q[0]; cp.exec_seed_base = (uint64_t)q[1]; cp.executions_per_test = (uint32_t)q[2];
    cp.tests_per_launch = (uint32_t)q[3]; cp.max_tests = (uint32_t)q[4];
    PUT_LONGS(campaign, cb, JNI_ABORT);
  }
  void* ev = BYTES(events);
  void* ar = LONGS(areasOrNull);
  jint rc = (LOST(events, ev) || LOST(areasOrNull, ar)) ? DEMI_ERR_INVALID_ARG
            : demi_fuzz_campaign_pipelined(CTX(h), &f.par, fieldGenOrNull ? &g : NULL, &cp, &pp, &lim, (demi_ext_event*)ev, (uint64_t*)ar,
                                           DEMI_MAX_EXT_EVENTS, &res, &st);
  PUT_LONGS(areasOrNull, ar, 0);
  PUT_BYTES(events, ev, 0);
  if (rc) return rc;
  o[0] = (jlong)res.found; o[1] = (jlong)res.test_index; o[2] = (jlong)res.exec_index; o[3] = (jlong)res.n_events; o[4] = (jlong)res.tests_run;
  o[5] = (jlong)res.launches; o[6] = (jlong)res.capacity_aborts;
  o[7] = (jlong)((uint64_t)res.verdict.flags | ((uint64_t)res.verdict.fingerprint << 32)); o[8] = (jlong)res.verdict.hash;
  SET_LONGS(result, 9, o);
  if (statsOrNull) {
    so[0] = (jlong)st.launches_submitted; so[1] = (jlong)st.launches_discarded;
    SET_LONGS(statsOrNull, 2, so);
  }
  return rc;
}
