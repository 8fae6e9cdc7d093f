package akka.dispatch.verification.gpu

/** JNI declarations, 1:1 with jni/demi_jni.c (which is 1:1 with include/demi_gpu.h).  Array layouts are documented at the
 *  top of demi_jni.c.  Every call returns 0 or a negative demi_status unless stated otherwise; lastError(h) has the text. */
object DemiGpu {
  System.loadLibrary("demi_jni")

  // DEMI_V_* verdict flags (include/demi_gpu.h)
  val V_VIOLATION = 0x1; val V_MAXMSG = 0x2; val V_PENDING_OVF = 0x4; val V_QUEUE_OVF = 0x8; val V_DIVERGED = 0x10
  val V_TRACE_OVF = 0x20; val V_PAIRS_OVF = 0x40; val V_SELFMSG = 0x80
  val MAX_PENDING = 128
  val MAX_REC_EVENTS = 16384
  val DPOR_ORDER_ROUNDS = 0; val DPOR_ORDER_REFERENCE = 1

  @native def ctxCreate(device: Int): Long
  @native def ctxDestroy(h: Long): Unit
  @native def lastError(h: Long): String
  @native def modelLoad(h: Long, nActors: Int, msgClass: Array[Byte], actorClass: Array[Byte], nClasses: Int,
                        handlerStart: Array[Short], code: Array[Int], initState: Array[Long], inv: Array[Int]): Int
  @native def modelSpecialize(h: Long, enable: Boolean): Int
  @native def traceLoad(h: Long, events: Array[Byte]): Int
  /** demi_ext_payload_areas: the 48-bit payload areas of the external events the NEXT traceLoad / dporLoad loads (a table whose
   *  messages have more than two fields: FlatEvents.packAreas); null forgets a staged array. */
  @native def extPayloadAreas(h: Long, areas: Array[Long]): Int
  @native def randomExplore(h: Long, seedBase: Long, n: Long, limits: Array[Int], verdicts: Array[Long]): Int
  @native def randomExploreFlagged(h: Long, seedBase: Long, n: Long, limits: Array[Int], flagMask: Int,
                                   out: Array[Long], counts: Array[Long]): Int
  /** explore() in pieces, up to three calls outstanding in one context (demi_random_explore_submit / _wait; the loop: submit(k + 2), wait(k)): the ticket (> 0) or a
   *  negative status; wait fills `out` / `counts` as randomExploreFlagged does */
  @native def randomExploreSubmit(h: Long, seedBase: Long, n: Long, limits: Array[Int], flagMask: Int): Int
  @native def randomExploreWait(h: Long, ticket: Int, out: Array[Long], counts: Array[Long]): Int
  /** returns the number of recorded events (16 bytes each in `recorded`: demi_rec_event), or a negative status */
  @native def randomGetTrace(h: Long, seed: Long, limits: Array[Int], verdict: Array[Long], recorded: Array[Byte]): Int
  /** the same for execution number `execIndex` of the instance seeded `seed` (demi_limits.executions_per_instance > 1) */
  @native def randomGetTraceCarried(h: Long, seed: Long, execIndex: Int, limits: Array[Int], verdict: Array[Long], recorded: Array[Byte]): Int
  @native def replayLoad(h: Long, externals: Array[Byte], recorded: Array[Byte]): Int
  @native def replayBatch(h: Long, masks: Array[Long], limits: Array[Int], verdicts: Array[Long]): Int
  /** replayBatch in pieces, up to three calls outstanding in one context (demi_replay_batch_submit / _wait; the loop: submit(k + 2), wait(k)): the ticket (> 0) or a
   *  negative status; `masks` may be reused as soon as submit returns.  wait: `n` is the submit's number of candidates, `verdictsOrNull` (long[2 * n]) receives every
   *  verdict, `out` / `counts` the flagged candidates as randomExploreFlagged fills them (index = the candidate's number within the call) */
  @native def replayBatchSubmit(h: Long, masks: Array[Long], limits: Array[Int], flagMask: Int, wantVerdicts: Boolean): Int
  @native def replayBatchWait(h: Long, ticket: Int, n: Long, verdictsOrNull: Array[Long], out: Array[Long], counts: Array[Long]): Int
  @native def replayRemovalBatch(h: Long, masksOrNull: Array[Long], skip: Array[Int], limits: Array[Int], verdicts: Array[Long]): Int
  /** RunnerUtils.stsSchedDDMin in one call (demi_ddmin): params = int[4] (depth, max_candidates, check_unmodified, verify_mcs), mcs = long[4],
   *  stats = long[5] (consultations, launches, mcs_len, verified, replays) */
  @native def ddmin(h: Long, limits: Array[Int], params: Array[Int], conjoinedOrNull: Array[Byte], mcs: Array[Long],
                    consultedOrNull: Array[Long], passedOrNull: Array[Byte], stats: Array[Long]): Int
  /** RunnerUtils.randomDDMin in one call (demi_random_ddmin) on the externals of traceLoad: params = int[6] (executions, depth, max_candidates,
   *  check_unmodified, verify_mcs, sequential), nExternals = how many externals traceLoad was given, mcs = long[4], stats = long[5]
   *  (consultations, launches, mcs_len, verified, executions run) */
  @native def randomDDMin(h: Long, seedBase: Long, limits: Array[Int], params: Array[Int], nExternals: Int, conjoinedOrNull: Array[Byte],
                          mcs: Array[Long], consultedOrNull: Array[Long], passedOrNull: Array[Byte], stats: Array[Long]): Int
  /** RandomScheduler.test for a batch of subsequences of the loaded externals (demi_random_explore_candidates): masks = long[4 * n],
   *  verdictsOrNull = long[2 * n * executions], flags = int[n] (bit 0 = some execution violates, bit 1 = some execution was aborted) */
  @native def randomExploreCandidates(h: Long, seedBase: Long, masks: Array[Long], executions: Int, limits: Array[Int],
                                      verdictsOrNull: Array[Long], flags: Array[Int]): Int
  /** Fuzz campaigns.  A Fuzzer crosses the boundary as numEvents, prefix / postfixOrNull = byte[8 * n] (demi_ext_event), weightBits =
   *  long[5] = doubleToRawLongBits of totalMass and the cumulative thresholds kill, + send, + partition, + unpartition (summed in
   *  FuzzerWeights' own order), gen = byte[136] (demi_fuzz_send_gen: the MessageGenerator as 1..8 alternatives (msg_type, target, p0, p1)).
   *  fuzzGenerate (demi_fuzz_generate): nTests tests, test i under new Random(seedBase + i) or seedsOrNull(i); they stay in the context;
   *  eventsOrNull = byte[8 * nTests * stride] with stride = prefix + numEvents + postfix + 1, nEv = int[nTests], nBatchesOrNull = int[nTests] */
  @native def fuzzGenerate(h: Long, numEvents: Int, prefix: Array[Byte], postfixOrNull: Array[Byte], weightBits: Array[Long], gen: Array[Byte],
                           seedBase: Long, seedsOrNull: Array[Long], nTests: Int, eventsOrNull: Array[Byte], nEv: Array[Int],
                           nBatchesOrNull: Array[Int]): Int
  /** one RandomScheduler run of `executions` executions per test, a workgroup per test (demi_random_explore_tests): testsOrNull =
   *  byte[8 * nTests * stride] with nEvOrNull = int[nTests], or null for the tests fuzzGenerate left in the context; verdictsOrNull =
   *  long[2 * nTests * executions]; flags = int[nTests] (bit 0 = some execution violates, bit 1 = some execution was aborted) */
  @native def randomExploreTests(h: Long, seedBase: Long, testsOrNull: Array[Byte], nEvOrNull: Array[Int], stride: Int, nTests: Int,
                                 executions: Int, limits: Array[Int], verdictsOrNull: Array[Long], flags: Array[Int]): Int
  /** RunnerUtils.fuzz's loop up to the first violating test (demi_fuzz_campaign): campaign = long[5] (test_seed_base, exec_seed_base,
   *  executions_per_test, tests_per_launch, max_tests), events = byte[8 * 255] (the violating test), result = long[9] (found, test_index,
   *  exec_index, n_events, tests_run, launches, capacity_aborts, verdict flags | fingerprint << 32, verdict hash) */
  @native def fuzzCampaign(h: Long, numEvents: Int, prefix: Array[Byte], postfixOrNull: Array[Byte], weightBits: Array[Long], gen: Array[Byte],
                           campaign: Array[Long], limits: Array[Int], events: Array[Byte], result: Array[Long]): Int
  /** The same for messages with more than two fields (a DEMI_MODEL_PAYLOADS table's external Sends): fieldGen = byte[296]
   *  (demi_fuzz_field_gen: 1..8 alternatives (msg_type, target, n_fields, kind[6], arg[6]); the draw order is the alternative, the target,
   *  then the fields 0, 1, .. in that order), and beside every array of events a long[] of as many 48-bit payload areas.
   *  fuzzGenerateFields (demi_fuzz_generate_fields): areasOrNull = long[nTests * stride]; events AND areas stay in the context */
  @native def fuzzGenerateFields(h: Long, numEvents: Int, prefix: Array[Byte], postfixOrNull: Array[Byte], weightBits: Array[Long],
                                 fieldGen: Array[Byte], seedBase: Long, seedsOrNull: Array[Long], nTests: Int, eventsOrNull: Array[Byte],
                                 areasOrNull: Array[Long], nEv: Array[Int], nBatchesOrNull: Array[Int]): Int
  /** randomExploreTests for any table (demi_random_explore_tests_areas): areasOrNull = long[nTests * stride] beside testsOrNull (null with
   *  tests: the areas are made of P0 / P1, as a load without staged areas does; testsOrNull = null: the resident events and areas) */
  @native def randomExploreTestsAreas(h: Long, seedBase: Long, testsOrNull: Array[Byte], areasOrNull: Array[Long], nEvOrNull: Array[Int],
                                      stride: Int, nTests: Int, executions: Int, limits: Array[Int], verdictsOrNull: Array[Long],
                                      flags: Array[Int]): Int
  /** fuzzCampaign with fieldGen (demi_fuzz_campaign_fields): areas = long[255], the violating test's payload areas beside its events */
  @native def fuzzCampaignFields(h: Long, numEvents: Int, prefix: Array[Byte], postfixOrNull: Array[Byte], weightBits: Array[Long],
                                 fieldGen: Array[Byte], campaign: Array[Long], limits: Array[Int], events: Array[Byte], areas: Array[Long],
                                 result: Array[Long]): Int
  /** One launch reduced on the device (demi_fuzz_launch_summary, then demi_fuzz_launch_summary_row): flagsOrNull = int[nTests] with
   *  verdictsOrNull = long[2 * nTests * executions], or both null for the results the last randomExploreTests(testsOrNull = null) left
   *  in the context - that call then takes verdictsOrNull = null and this one is read instead of its flags.  result = long[8] (first_hit,
   *  capacity_aborts, exec_index, aborted_before, n_events, 0, verdict flags | fingerprint << 32, verdict hash); eventsOrNull = byte[8 * 255]
   *  and areasOrNull = long[255] receive the violating test of the resident form. */
  @native def fuzzLaunchSummary(h: Long, flagsOrNull: Array[Int], verdictsOrNull: Array[Long], nTests: Int, executions: Int,
                                eventsOrNull: Array[Byte], areasOrNull: Array[Long], result: Array[Long]): Int
  /** fuzzCampaign / fuzzCampaignFields with up to inFlight launches on the device at a time (demi_fuzz_campaign_pipelined; inFlight 1..3,
   *  0 = 2): exactly one of gen (byte[136]) and fieldGen (byte[296]) is non-null; areasOrNull = long[255] with fieldGen; result as
   *  fuzzCampaign's; statsOrNull = long[2] (launches_submitted, launches_discarded).  The same answers as the synchronous calls. */
  @native def fuzzCampaignPipelined(h: Long, numEvents: Int, prefix: Array[Byte], postfixOrNull: Array[Byte], weightBits: Array[Long],
                                    genOrNull: Array[Byte], fieldGenOrNull: Array[Byte], campaign: Array[Long], inFlight: Int,
                                    limits: Array[Int], events: Array[Byte], areasOrNull: Array[Long], result: Array[Long],
                                    statsOrNull: Array[Long]): Int
  @native def replayGetKept(h: Long, maskOrNull: Array[Long], skip: Int, limits: Array[Int], verdict: Array[Long], kept: Array[Byte]): Int
  /** one round of STSSchedMinimizer.minimize, reduced on the device (demi_replay_removal_round): skip = the strategy's upcoming proposals,
   *  kept = byte[n recorded] (the executed-trace marks of proposal first_hit), result = long[6] (first_hit or -1, n_kept, retried, launches,
   *  the winner's two verdict words) */
  @native def replayRemovalRound(h: Long, maskOrNull: Array[Long], skip: Array[Int], limits: Array[Int], kept: Array[Byte], result: Array[Long]): Int
  /** RunnerUtils.minimizeInternals in one call (demi_minimize_internals) on the execution replayLoad loaded, which is the minimized one
   *  afterwards: params = int[2] (strategy: 0 LeftToRightOneAtATime, 1 SrcDstFIFORemoval; max_batch), trace = byte[16 * cap] (the minimized
   *  recorded events), sizesOrNull = int[] (record_internal_size per replay), stats = long[10] (events of the result, total_replays,
   *  replays_run, rounds, launches, adoptions, retried, unignorable, deliveries_before, deliveries_after) */
  @native def minimizeInternals(h: Long, limits: Array[Int], params: Array[Int], trace: Array[Byte], sizesOrNull: Array[Int], stats: Array[Long]): Int
  /** the selectors of the execution replayLoad loaded (demi_replay_wildcard_load): typeSets = int[n recorded] (bit t = message type t
   *  matches, 0 = exact delivery), policies = byte[n recorded] (0 HEAD = SrcDstFIFOOnly, 1 FIRST = BackTrackStrategy / the timer wildcard,
   *  2 LAST = LastOnlyStrategy) */
  @native def replayWildcardLoad(h: Long, typeSets: Array[Int], policies: Array[Byte]): Int
  /** one STSScheduler.test of a wildcarded trace per row (demi_replay_wildcard_batch): present = long[ceil(n recorded / 64) * n],
   *  bit i of a row = the MsgEvent recorded at i is part of the trace; verdicts = long[2 * n] */
  @native def replayWildcardBatch(h: Long, masksOrNull: Array[Long], present: Array[Long], limits: Array[Int], verdicts: Array[Long]): Int
  /** one candidate once more, recorded (demi_replay_wildcard_get_trace): returns the number of events of the executed trace in
   *  `recorded` (16 bytes each), or a negative status; kept = byte[n recorded] */
  @native def replayWildcardGetTrace(h: Long, maskOrNull: Array[Long], present: Array[Long], limits: Array[Int], verdict: Array[Long],
                                     kept: Array[Byte], recorded: Array[Byte]): Int
  /** one round of WildcardMinimizer.doMinimize, reduced on the device (demi_replay_wildcard_round): present = long[ceil(n recorded / 64) * n],
   *  the clusterizer's n upcoming proposals; kept = byte[n recorded] (the executed-trace marks of proposal first_hit); result = long[8]
   *  (first_hit or -1, executed_len, n_kept, retried, launches, 0, the winner's two verdict words) */
  @native def replayWildcardRound(h: Long, maskOrNull: Array[Long], present: Array[Long], n: Int, limits: Array[Int], kept: Array[Byte],
                                  result: Array[Long]): Int
  /** WildcardMinimizer.minimize in one call (demi_minimize_wildcards) on the execution replayLoad loaded, which is the minimized one
   *  afterwards (no selectors; the call lowers its own): params = int[5] (clustering: 0 ClockClusterizer, 1 SingletonClusterizer,
   *  2 ClockThenSingleton; policy: 0 HEAD, 1 FIRST, 2 LAST; skipClockClusters; max_batch; clock-increment types, bit t), clockField =
   *  byte[32] (payload field of getLogicalClock per message type, -1: none), trace = byte[16 * cap], sizesOrNull = int[]
   *  (record_internal_size per replay and the fencepost), stats = long[10] (events of the result, total_replays, replays_run, rounds,
   *  launches, adoptions, retried, entries of sizes, deliveries_before, deliveries_after) */
  @native def minimizeWildcards(h: Long, limits: Array[Int], params: Array[Int], clockField: Array[Byte], trace: Array[Byte],
                                sizesOrNull: Array[Int], stats: Array[Long]): Int
  /** one WildcardTestOracle.test per candidate (demi_replay_wildcard_candidates): masks = long[4 * n]; proposal 0 = basePresentOrNull
   *  (null: every delivery), proposal j = that row without the MsgEvent recorded at drops(j - 1); out = long[3 * n]
   *  (first_hit | executed_len << 32, flags | first_ovf << 32, hash; flags: 1 reproduces, 2 unknown because of a capacity, 4 longer than
   *  the loaded trace); outAllOrNull = long[2 * n * (1 + drops.length)] */
  @native def replayWildcardCandidates(h: Long, masks: Array[Long], basePresentOrNull: Array[Long], drops: Array[Int], limits: Array[Int],
                                       out: Array[Long], outAllOrNull: Array[Long]): Int
  /** RunnerUtils.wildcardDDMin in one call (demi_wildcard_ddmin): params, conjoinedOrNull, mcs, consultedOrNull / passedOrNull and stats as
   *  for ddmin; firstHitOrNull = int[cap] (-1: no proposal reproduced); result = long[13] (total_replays, proposals_run, mcs_evaluated,
   *  mcs_first_hit (-1: none), mcs_executed_len, mcs_flags, retried, min_first_hit (-1: none), min_executed_len, min_externals[4]:
   *  WildcardTestOracle's minTrace / externalsForMinTrace after the search) */
  @native def wildcardDDMin(h: Long, limits: Array[Int], params: Array[Int], conjoinedOrNull: Array[Byte], basePresentOrNull: Array[Long],
                            drops: Array[Int], mcs: Array[Long], consultedOrNull: Array[Long], passedOrNull: Array[Byte],
                            firstHitOrNull: Array[Int], stats: Array[Long], result: Array[Long]): Int
  @native def dporLoad(h: Long, externals: Array[Byte]): Int
  /** returns the length of the first violating trace (entries of 16 bytes in firstViolationTrace), or a negative status */
  /** ArvindDistanceOrdering.init(sched, originalTrace) / setInitialTrace for the following dporExplore calls (node keys; 16-byte trace entries) */
  @native def dporSetTraces(h: Long, originalKeysOrNull: Array[Long], initialTraceOrNull: Array[Byte]): Int
  @native def dporExplore(h: Long, params: Array[Int], search: Array[Int], verdicts: Array[Long], prefixLen: Array[Int],
                          rounds: Array[Int], firstViolationTrace: Array[Byte], stats: Array[Long]): Int
  /** What interleaving `index` of the last dporExplore was (demi_dpor_explored): nextTrace / trace = byte[16 * 256] (16-byte trace entries),
   *  lens = long[3] (next-trace length, its shared take() part, executed-trace length).  For diffing an exploration against DPORwHeuristics. */
  @native def dporExplored(h: Long, index: Long, nextTrace: Array[Byte], trace: Array[Byte], lens: Array[Long]): Int
  /** n interleavings whose next traces hold wildcards, one launch (demi_dpor_wildcard_batch; DPORwHeuristics.scala:474-514): 16-byte
   *  entries of kind 3 (a WildCardMatch: key = type set | policy << 32 | backtrack mode << 40) and 4 (Unique(_, -1) of an external
   *  message, by word) beside kinds 0 / 1 / 2.  verdicts long[2 * n]; traces byte[16 * 256 * n]; ignored / wild long[4 * n]: 256 bits
   *  each (ignoreAbsentCallback positions; trace entries a wildcard picked); alts byte[16 * maxAlts * n] (key, word, trace length,
   *  position, producer index), nAlts int[n] */
  @native def dporWildcardBatch(h: Long, prefixes: Array[Byte], prefixLen: Array[Int], stride: Int, params: Array[Int],
                                stopAfterNextTrace: Boolean, maxAlts: Int, verdicts: Array[Long], traces: Array[Byte], traceLen: Array[Int],
                                ignored: Array[Long], wild: Array[Long], alts: Array[Byte], nAlts: Array[Int]): Int
  /** WildcardMinimizer.testWithDpor of one proposal in one call (demi_wildcard_dpor_test, WildcardMinimizer.scala:67-114): initial =
   *  the proposal's uniques as 16-byte entries; params = int[7] (max_messages = uniques.size); wc = int[3] (dpor_budget - interleavings,
   *  the reference's budgetSeconds as a count -, batch, max_alts); trace = byte[16 * 256]; result = long[16] (hit, interleavings,
   *  speculated, launches, exhausted, budget_reached, retried, trace_len, skipped_explored, points, 0, 0, ignored[0 .. 3]) */
  @native def wildcardDporTest(h: Long, initial: Array[Byte], params: Array[Int], wc: Array[Int], trace: Array[Byte], result: Array[Long]): Int
  /** RunnerUtils.editDistanceDporDDMin in one call (demi_edit_distance_dpor_ddmin: IncrementalDDMin over ResumableDPOR, every DPOR
   *  consultation inside the library).  externals = 8 bytes each; initialTrace = 16-byte entries (FlatEvents.dporInitialTrace);
   *  dporParams = int[7]; params = int[7] (max_max_distance, stop_at_size, check_unmodified, ignore_quiescence, verify_mcs, batch, budget);
   *  mcs = long[4]; consultedOrNull = long[4 * cap] with passedOrNull = byte[cap], distanceOrNull = int[cap];
   *  violationTraceOrNull = byte[16 * 256]; stats = long[40] (replays, interleavings, consultations, instances, passes, mcs_len, verified,
   *  violation_len, pass_distance[16], pass_mcs_len[16]) */
  @native def editDistanceDporDDMin(h: Long, externals: Array[Byte], initialTrace: Array[Byte], dporParams: Array[Int], params: Array[Int],
                                    mcs: Array[Long], consultedOrNull: Array[Long], passedOrNull: Array[Byte], distanceOrNull: Array[Int],
                                    violationTraceOrNull: Array[Byte], stats: Array[Long]): Int
  /** ProvenanceTracker.pruneConcurrentEvents for n traces (16-byte entries, `stride` per trace); keep: 4 longs (256 bits) per trace */
  @native def provenancePrune(h: Long, traces: Array[Byte], traceLen: Array[Int], affected: Array[Int], stride: Int, keep: Array[Long]): Int
  @native def commUniqueId(id128: Array[Byte]): Int
  @native def commCreate(h: Long, id128: Array[Byte], rank: Int, world: Int): Int
  @native def commDestroy(h: Long): Int
  @native def randomExploreSharded(h: Long, seedBase: Long, nTotal: Long, limits: Array[Int], out: Array[Long], count: Array[Long]): Int

  def check(h: Long, rc: Int): Int = { if (rc < 0) throw new RuntimeException("demi_gpu error " + rc + ": " + lastError(h)); rc }
  def flags(verdicts: Array[Long], i: Int): Int = (verdicts(2 * i) & 0xFFFFFFFFL).toInt
  def fingerprint(verdicts: Array[Long], i: Int): Int = (verdicts(2 * i) >>> 32).toInt
  def hash(verdicts: Array[Long], i: Int): Long = verdicts(2 * i + 1)
}
