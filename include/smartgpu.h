/*
 * smartgpu.h — C ABI of the MI355X exact-string-matching engine that sits
 * behind SMART's per-algorithm plugin surface.
 *
 * Drop-in boundary.  Each entry point names the reference
 * interface it replaces (paths relative to the SMART tree):
 *
 *   reference                                      this library
 *   ---------------------------------------------  ---------------------------------
 *   int search(unsigned char*,int,unsigned char*,  smartgpu_<algo>_search()   (same shape,
 *       int)          src/algos/include/main.h:39    same return convention: count, -1 = n/a)
 *   double *run_time,*pre_time (ms, written by the  smartgpu_last_times(), and the pre_ms /
 *       BEGIN_/END_ macros)   main.h:28-31,34-35    run_ms out-params of smartgpu_search64()
 *   text in a SysV segment: shmget(tkey,TSIZE+10)   smartgpu_text_upload()/_generate()/_free():
 *       + getText()    src/smart.c:553-568,95-138    the text lives in HBM for a whole run
 *   execute(): system("./source/bin/<algo> shared   smartgpu_search64() — an in-process call
 *       ...")          src/smart.c:140-146           instead of a process spawn per pattern
 *   textgen rand-sigma corpora  src/textgen.c:34-54 smartgpu_text_generate() (on-device,
 *                                                    counter-based)
 *
 * All pointers are plain host pointers unless a parameter says "device"; there
 * are no C++ or torch types in any signature.  The library is single-threaded
 * from the caller's point of view (like SMART); every call that returns a count
 * is synchronous.  Errors: negative return codes, text in smartgpu_last_error().
 * Threading contract: ONE host thread per device at a time — the per-device stream, staging buffer and table arena are
 * shared by every call on that device (src/smart.c is single-threaded); last_error / last_times are
 * thread-local.  Loading the library sets HSA_ENABLE_IPC_MODE_LEGACY=0 (unless the environment already has it) so that
 * RCCL works on hosts that only support dmabuf IPC: load it before the process makes its first HIP call.
 *
 * There is no CPU fallback: without a usable HIP device every compute entry
 * point fails with SMARTGPU_ERR_HIP.
 */
#ifndef SMARTGPU_H
#define SMARTGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMARTGPU_XSIZE 4200 /* longest pattern, src/algos/include/define.h:25 */

/* return codes (SMART keeps count>=0 / -1 "not applicable"; src/smart.c:143-145,330-343) */
#define SMARTGPU_OK 0
#define SMARTGPU_NA (-1)          /* algorithm not applicable / count does not fit an int */
#define SMARTGPU_ERR_ARG (-3)     /* bad argument (unknown algorithm, m<1, m>XSIZE, range) */
#define SMARTGPU_ERR_HIP (-4)     /* HIP runtime error or no device */
#define SMARTGPU_ERR_NOMEM (-5)

/* algorithm ids; names are SMART's lower-case executable names (src/smart.c:142) */
enum {
    SMARTGPU_HOR = 0,  /* src/algos/hor.c  */
    SMARTGPU_BM = 1,   /* src/algos/bm.c   */
    SMARTGPU_KMP = 2,  /* src/algos/kmp.c  */
    SMARTGPU_SO = 3,   /* src/algos/so.c   */
    SMARTGPU_BNDM = 4, /* src/algos/bndm.c */
    SMARTGPU_EPSM = 5, /* src/algos/epsm.c */
    /* adjacent algorithm names on the same engine */
    SMARTGPU_SA = 6,      /* src/algos/sa.c      Shift-And, the dual of so.c            */
    SMARTGPU_QS = 7,      /* src/algos/qs.c      Quick Search: shift on the byte after the window */
    SMARTGPU_TUNEDBM = 8, /* src/algos/tunedbm.c Horspool's table with a zero entry + skip loop   */
    SMARTGPU_RAITA = 9,   /* src/algos/raita.c   Horspool's shifts, last/middle/first/rest order; m >= 2 (raita.c:37) */
    SMARTGPU_HASH3 = 10,  /* src/algos/hash3.c   Lecroq: shift under an 8-bit hash of the last 3 bytes; m >= 3 */
    SMARTGPU_HASH5 = 11,  /* src/algos/hash5.c   ... of the last 5 bytes; m >= 5 */
    SMARTGPU_HASH8 = 12,  /* src/algos/hash8.c   ... of the last 8 bytes; m >= 8 */
    SMARTGPU_SBNDM = 13,  /* src/algos/sbndm.c   Simplified BNDM; m >= 2 */
    SMARTGPU_KR = 14,     /* src/algos/kr.c      Karp-Rabin: rolling 32-bit hash + confirmation */
    SMARTGPU_BNDML = 15,  /* src/algos/bndml.c   BNDM with multi-word bit vectors for m > 32 */
    SMARTGPU_NUM_ALGOS = 16
};

typedef struct smartgpu_text smartgpu_text; /* a text resident in one GPU's HBM */
typedef struct smartgpu_plan smartgpu_plan; /* one (algorithm, pattern) with its tables in HBM */

/* ---- library ---------------------------------------------------------- */
const char *smartgpu_version(void);
const char *smartgpu_last_error(void);
int smartgpu_device_count(void);                   /* <0 on error */
int smartgpu_algo_id(const char *name);            /* "hor","bm","kmp","so","bndm","epsm","sa","qs","tunedbm","raita","hash3","hash5","hash8","sbndm","kr","bndml" (any case); -1 unknown */
const char *smartgpu_algo_name(int algo);          /* NULL if out of range */
int smartgpu_device_sync(int device);              /* waits for the library's stream on `device` */

/* ---- text lifecycle (replaces shmget + getText, src/smart.c:553-568,95-138) ---- */
/* Copies host[0..n) into HBM of `device` through pinned staging.  NULL on error. */
smartgpu_text *smartgpu_text_upload(const void *host, uint64_t n, int device);
/* Text byte i = unit[(phase + i) % unit_len] for i in [0,n): a corpus replicated
 * to a target size (BASELINE config 4) without shipping n bytes over PCIe. */
smartgpu_text *smartgpu_text_upload_tiled(const void *unit, uint64_t unit_len, uint64_t phase,
                                          uint64_t n, int device);
/* Text byte i = byte (off+i) of the counter-based rand-sigma corpus, generated on
 * the device: splitmix64(seed + (j>>3)) >> (8*(j&7)), masked (sigma a power of
 * two) or reduced modulo sigma.  2 <= sigma <= 256. */
smartgpu_text *smartgpu_text_generate(uint64_t seed, int sigma, uint64_t off, uint64_t n, int device);
void smartgpu_text_free(smartgpu_text *t);
uint64_t smartgpu_text_length(const smartgpu_text *t);
int smartgpu_text_device(const smartgpu_text *t);
/* Copies text[off..off+len) back to the host (tests, pattern extraction à la
 * setOfRandomPatterns, src/smart.c:148-158). */
int smartgpu_text_read(const smartgpu_text *t, uint64_t off, uint64_t len, void *host);
/* Which byte values the text holds: bit c of bits[8] (bit c%32 of word c/32) is set iff some text byte equals c.
 * Taken once, on the device, when the text is created (the reference's getText, src/smart.c:95-138, reads the corpus
 * once per run as well; a text is never written afterwards).  The runs kernels use it: on a text of at most four
 * distinct values they take four bytes per table step. */
int smartgpu_text_alphabet(const smartgpu_text *t, uint32_t bits[8]);
/* How often two symbols of the text are equal: sum c (c - 1) / (N (N - 1)) over the byte histogram of a sample of N
 * bytes, taken on the device in the same pass as the alphabet — 16-byte chunks at an even stride, at most 2^20 of
 * them; a text of up to 16 MiB is counted whole.  rand128 gives 1/128, rand32 1/32, English about 0.066.  *rate is -1
 * where there is none: an empty or one-byte text, or one that the plugin-shape calls below upload for a single search.
 * smartgpu_plan_launch() asks it before a pattern whose own symbols repeat may share a pass. */
int smartgpu_text_repeat_rate(const smartgpu_text *t, double *rate);

/* ---- searching -------------------------------------------------------- */
/* Counts the occurrences of P[0..m) whose window lies inside text[off..off+n),
 * i.e. start positions s in [off, off+n-m].  Overlapping occurrences count
 * (define.h:33).  *pre_ms = host table construction + table upload
 * (BEGIN_/END_PREPROCESSING, main.h:28,30); *run_ms = kernel(s) + count readback,
 * by HIP events (BEGIN_/END_SEARCHING, main.h:29,31).  Either may be NULL. */
int smartgpu_search64(int algo, const uint8_t *P, uint32_t m, const smartgpu_text *text,
                      uint64_t off, uint64_t n, uint64_t *count, double *pre_ms, double *run_ms);

/* The harness's inner loop as ONE call (src/smart.c:312-345: for each of the -pset patterns of a length,
 * execute() and read count and times back): K patterns of m bytes each, P[0..K), over the same resident
 * text range.  Preprocessing: the K tables are built on the host and placed in one arena in HBM (grown
 * when a batch needs more, never allocated per pattern); searching: K launches back to back on the
 * device's stream and ONE read-back of the K counts, so the synchronous per-call cost of
 * smartgpu_search64 (25-30 us) is paid once per pattern set.  On texts up to 32 MiB the patterns whose plans
 * choose the same kernel share one grid (gridDim.y = pattern, at most 65535 per grid: a larger group is
 * launched in slices).  K is at most 262144 (2^18) per call: SMARTGPU_ERR_ARG beyond.
 *   counts[k]   occurrences of P[k]                                   (K entries, required)
 *   pre_ms[k]   host table construction of P[k] + its share of the upload     (K entries or NULL)
 *   run_ms[k]   device time of the k-th search by HIP events — one event per pattern — (K entries or NULL:
 *               no per-pattern events)
 *   *batch_ms   wall clock from the first launch to the counts on the host   (or NULL)              */
int smartgpu_search_batch64(int algo, const uint8_t *const *P, uint32_t m, uint32_t K, const smartgpu_text *text,
                            uint64_t off, uint64_t n, uint64_t *counts, double *pre_ms, double *run_ms,
                            double *batch_ms);
/* The same, with EVERY pattern launched on its own between its own pair of events, whatever the text's size: run_ms[k]
 * is then pattern k's device time alone (in the one-grid form above a group's patterns share their group's time).  What
 * the harness uses when best / worst / standard deviation or the -tb bound are asked for: src/smart.c:320-329 times
 * every pattern, :337-343 applies the bound per run, :347-351 derives best, worst and std from those times. */
int smartgpu_search_batch64_each(int algo, const uint8_t *const *P, uint32_t m, uint32_t K, const smartgpu_text *text,
                            uint64_t off, uint64_t n, uint64_t *counts, double *pre_ms, double *run_ms,
                            double *batch_ms);

/* SMART's own plugin shape, one symbol per algorithm (main.h:39).  T is a HOST
 * pointer: the text is uploaded for the call and released afterwards, so this
 * is the compatibility path, not the fast one.  Returns the count, or -1 when
 * it does not fit an int / on error (smart.c:143-145 maps any failure to -1). */
int smartgpu_hor_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_bm_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_kmp_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_so_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_bndm_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_epsm_search(const unsigned char *P, int m, const unsigned char *T, int n);
int smartgpu_sa_search(const unsigned char *P, int m, const unsigned char *T, int n);      /* sa.c:36-94 */
int smartgpu_qs_search(const unsigned char *P, int m, const unsigned char *T, int n);      /* qs.c:33-52 */
int smartgpu_tunedbm_search(const unsigned char *P, int m, const unsigned char *T, int n); /* tunedbm.c:36-65 */
int smartgpu_raita_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* raita.c:35-64; -1 for m < 2 */
int smartgpu_hash3_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* hash3.c:28-84; -1 for m < 3 */
int smartgpu_hash5_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* hash5.c; -1 for m < 5 */
int smartgpu_hash8_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* hash8.c; -1 for m < 8 */
int smartgpu_sbndm_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* sbndm.c:28-149; -1 for m < 2 */
int smartgpu_kr_search(const unsigned char *P, int m, const unsigned char *T, int n);      /* kr.c:28-54 */
int smartgpu_bndml_search(const unsigned char *P, int m, const unsigned char *T, int n);   /* bndml.c:44-132 */
/* pre/run times (ms) of the last search on this thread (main.h:34-35 globals) */
void smartgpu_last_times(double *pre_ms, double *run_ms);

/* ---- occurrence positions (extension) -------------------------- */
/* The reference only counts (OUTPUT(j) is count++, define.h:33).  This call also returns WHERE:
 * every s in [off, off+n-m] with T[s..s+m) == P, ascending, relative to text byte 0, through the
 * packed matcher with an output stage.  positions is a HOST buffer of `cap` entries.
 * *count always receives the number of occurrences.  Returns SMARTGPU_OK when count <= cap (the
 * list is complete), SMARTGPU_ERR_NOMEM when it is not (retry with cap >= *count). */
int smartgpu_find64(const uint8_t *P, uint32_t m, const smartgpu_text *text, uint64_t off, uint64_t n,
                    uint64_t *positions, uint64_t cap, uint64_t *count);
/* The positions of a whole PATTERN SET of one length, in shared passes over the text: smartgpu_pfind_batch64's contract
 * (below), asked of a smartgpu_text.  The positions of pattern k are positions[starts[k] .. starts[k+1]), each slice
 * ascending and relative to text byte 0: every s in [off, off+n-m] with T[s..s+m) == P[k], overlapping occurrences
 * listed.  starts has K+1 entries, starts[0] = 0, starts[K] = the total.  starts[K] > cap: SMARTGPU_ERR_NOMEM with
 * starts completely filled — every count and the room a retry needs.  cap == 0 with positions == NULL is a count.
 * Nothing behind positions[cap] is ever written.  m > n leaves all counts 0 without a launch.  The same pattern twice
 * in a set gets two equal slices.
 * One kernel, hor_multi_find (smart_amd/csrc/k_hormf.hip): hor_multi_scan's skip table, walk and candidate chains
 * with an output stage.  A pass decides 208 patterns up to m = 16, 124 up to m = 32, 89 up to m = 48, 69 up to
 * m = 64 and 56 beyond in ONE read of the text, and it counts and lists in the same read, so starts is exact even
 * when entries were dropped; the passes of a call run back to back, with one synchronisation and one copy to the host.
 * m = 1 and m = 2 have no two-byte gram to skip on: they are answered by K runs of smartgpu_find64 into consecutive
 * slices, under the same contract.
 * SMARTGPU_ERR_ARG, each decided before any HIP call: the argument checks of smartgpu_search_batch64; starts == NULL;
 * positions == NULL with cap > 0; a NULL pattern; K > 262144 (2^18: an entry keeps 18 bits for the pattern);
 * K > SMARTGPU_FIND_BATCH_STAGING / (bytes staged per pattern) — the patterns travel through the device's pinned
 * staging buffer, 16 * ceil(min(m, 65) / 16) bytes of a pattern's end and, from m = 18 on, 16 * ceil(m / 16) of the
 * whole pattern: 87381 patterns at m = 300, 8035 at m = 4096, no bound below 2^18 up to m = 64; off + n >= 2^46 (an
 * entry keeps 46 bits for the position).  What the device wrote is refused with SMARTGPU_ERR_HIP, never reported,
 * where its cursor and its counts disagree or the entries are not the counted occurrences.
 * NOT offered: patterns of several lengths in one call (smart_amd.find_batch groups them by length), MultiText shards.
 * Measured with tools/find_batch_probe.py (profiles/coalesce/RESULTS.md, "Positions of a pattern set"). */
#define SMARTGPU_FIND_BATCH_STAGING (32u << 20)
int smartgpu_find_batch64(const uint8_t *const *P, uint32_t m, uint32_t K, const smartgpu_text *text,
                          uint64_t off, uint64_t n, uint64_t *positions, uint64_t cap, uint64_t *starts);

/* ---- plans: preprocess once, launch many (harness hot loop, smart.c:312-345) ---- */
/* Builds the algorithm's tables on the host and places them in HBM of `device`. */
smartgpu_plan *smartgpu_plan_create(int algo, const uint8_t *P, uint32_t m, int device);
void smartgpu_plan_free(smartgpu_plan *p);
/* Hands one search of text[off..off+n) to the device's stream and returns
 * without waiting; the count is ADDED to result slot `slot` (0 <= slot < 4096)
 * of the plan (slots start at zero; smartgpu_plan_reset() zeroes them again).
 * With `timed` != 0 the launch is bracketed by HIP events.
 * Untimed streaming Horspool / Tuned BM launches over one range of one text with
 * one pattern length may be held back until smartgpu_coalesce() of them have
 * gathered and then run as ONE pass over the text (hor_multi_scan); the counts
 * are the same; launches that are held back may run after later launches that are
 * not (counts are added, so the order decides nothing).  A pattern whose own symbols
 * repeat (it would run on hor_scan's verifying form, alone) is held back as well where
 * the TEXT's symbols do not — smartgpu_text_repeat_rate() at most 1/48 — and a key is
 * already gathering for its text, range and length: it rides in that key's pass, opens
 * none of its own and does not count toward smartgpu_coalesce(); with no such key, on
 * any other text, or timed, it is sent at once as before.  A launch is complete no later than the next
 * smartgpu_device_sync(), smartgpu_plan_result() or smartgpu_stream_mark() on its
 * device; every other call that waits for, times, resets or frees what the launch
 * touches sends it first as well.  A caller who synchronises by other means (the
 * stream of smartgpu_stream_handle(), which switches this off for its device, or
 * a device-wide synchronisation of their own) calls smartgpu_coalesce(0). */
int smartgpu_plan_launch(smartgpu_plan *p, const smartgpu_text *text, uint64_t off, uint64_t n,
                         int slot, int timed);
/* Waits for the stream and returns the count of `slot` (and, if the launch was
 * timed, its device time in ms; else *kernel_ms = -1). */
int smartgpu_plan_result(smartgpu_plan *p, int slot, uint64_t *count, double *kernel_ms);
/* Name of the dominant kernel the plan launches (as rocprofv3 reports it). */
const char *smartgpu_plan_kernel_name(const smartgpu_plan *p);
/* The same for (algo, P, m) without a device: which kernel a plan of this pattern would launch under the
 * current smartgpu_tune() settings — the host-side choice (DESIGN.md §4 "The plan reads the pattern").  NULL
 * if algo or m is out of range. */
const char *smartgpu_kernel_for(int algo, const uint8_t *P, uint32_t m);
/* Device address of the plan's uint64 result slots (for an RCCL reduce issued
 * by the caller on the same device). */
void *smartgpu_plan_result_device_ptr(smartgpu_plan *p);
/* Zeroes every result slot (stream-ordered). */
int smartgpu_plan_reset(smartgpu_plan *p);
/* Makes the plan write its counts to caller-owned DEVICE memory (`nslots`
 * uint64, zeroed by the caller), e.g. one element of a vector that the caller
 * reduces across GPUs with RCCL.  NULL restores the plan's own slots. */
int smartgpu_plan_set_result_buffer(smartgpu_plan *p, void *device_u64, int nslots);

/* ---- one process, several GPUs (the 8 GPUs of a node) ---------------------------- */
/* A text sharded by byte offset over `ngpus` devices of this process: device g owns the
 * start positions [g*n/k, (g+1)*n/k) and holds SMARTGPU_XSIZE extra bytes, so any pattern
 * length can be searched without an exchange step.  `devices` lists the
 * device ordinals (NULL = 0..ngpus-1). */
typedef struct smartgpu_mtext smartgpu_mtext;
smartgpu_mtext *smartgpu_mtext_upload(const void *host, uint64_t n, int ngpus, const int *devices);
smartgpu_mtext *smartgpu_mtext_generate(uint64_t seed, int sigma, uint64_t n, int ngpus, const int *devices);
void smartgpu_mtext_free(smartgpu_mtext *t);
uint64_t smartgpu_mtext_length(const smartgpu_mtext *t);
int smartgpu_mtext_ngpus(const smartgpu_mtext *t);
/* The partition itself (pure arithmetic, no device): shard g of `ngpus` over a text of n bytes owns the start positions
 * [*begin, *begin + *own) — the shards' sizes differ by at most one byte and add up to n — and holds *held bytes from
 * *begin on: its own and up to SMARTGPU_XSIZE - 1 of the following shards', never beyond byte n.  Any pointer may be NULL. */
int smartgpu_mtext_partition(uint64_t n, int ngpus, int g, uint64_t *begin, uint64_t *own, uint64_t *held);
/* Self-test of the host-thread pool that enqueues the k devices' launches of a multi-GPU search at once (no device
 * needed): `rounds` rounds of up to k jobs, each job must run exactly once per round.  0 = passed. */
int smartgpu_selftest_launch_pool(int k, int rounds);
/* Searches every shard concurrently (one stream per device) and sums the shard counts.
 * reduce = SMARTGPU_REDUCE_RCCL: ncclAllReduce(sum, uint64) over the devices' streams (RCCL
 * over xGMI; the devices must be distinct), then one 8-byte read-back;
 * reduce = SMARTGPU_REDUCE_HOST: eight-byte read-backs added on the host (also allows the
 * same device to appear more than once, which is how the shard arithmetic is tested on a
 * one-GPU box).  *run_ms covers launches + reduction + read-back. */
#define SMARTGPU_REDUCE_RCCL 0
#define SMARTGPU_REDUCE_HOST 1
int smartgpu_msearch64(int algo, const uint8_t *P, uint32_t m, smartgpu_mtext *text, int reduce,
                       uint64_t *count, double *pre_ms, double *run_ms);

/* The pattern-set form of smartgpu_msearch64: every device searches its shard for all K patterns, then ONE
 * reduction of the K counts (RCCL: one ncclAllReduce of K uint64 per device, in place) and one read-back. */
int smartgpu_msearch_batch64(int algo, const uint8_t *const *P, uint32_t m, uint32_t K, smartgpu_mtext *text,
                             int reduce, uint64_t *counts, double *pre_ms, double *batch_ms);

/* ---- stream timing (hipEvents on the stream the kernels run on) ------------ */
int smartgpu_stream_mark(int device, int which /* 0 = begin, 1 = end */);
int smartgpu_stream_elapsed_ms(int device, double *ms); /* waits for mark 1 */
void *smartgpu_stream_handle(int device);               /* hipStream_t of the library on `device` */

/* Measures the device's practical streaming-read rate on this text (a plain
 * coalesced read-and-fold kernel, `reps` passes): the "measured streaming read"
 * the scan kernels are compared with besides the 8 TB/s spec peak. */
int smartgpu_probe_read_ms(const smartgpu_text *t, int reps, double *ms_per_pass);

/* Kernel-variant selection for experiments and A/B measurements (not needed in normal use;
 * every variant is parity-tested).  Keys:
 *   0  regime of the skip algorithms: 0 auto — short patterns and patterns whose symbols repeat on
 *      the packed matcher, patterns of 16+ bytes over two or three symbols on so_runs, the rest on
 *      the algorithm's own LDS-tile skip loop / 1 always the algorithm's own skip
 *      loop / 2 Horspool's bank-private LDS layout / 3 always the packed matcher
 *   1  bndm_scan: bytes of a window read per iteration (1, 2, 4, 8; 0 = the plan's choice from the pattern);
 *      9 = the plan's choice and never the gram form of texts of at most four byte values (round 4)
 *   2  bm_scan / bndm_scan workgroups: 1 four waves / 2 two waves (0 = default: bm_scan two where the pattern's symbols
 *      repeat, bndm_scan always four); 3 = Horspool's nested loop also where the pattern's symbols repeat (default
 *      there: its flat form, round 3); 4 = Horspool, Tuned BM and Boyer-Moore never on grams (round 4: hor_scan_gram,
 *      bm_scan_gram on texts of at most four byte values)
 *   4  workgroups per CU of the LDS-tile kernels (0 = the launcher's choice)
 *   3  KMP: 0 kmp_runs (transition table) / 1 kmp_scan (LDS tiles, m <= 40) / 2 kmp_links_runs
 *      (failure links followed per byte) / 5 kmp_runs a byte per table step even on a text of at most four
 *      byte values (round 3: there it takes four) / 6 round 3's one-workgroup-per-CU form (round 4: five compact
 *      workgroups per CU; key 4 sets their number)
 *   5  run length in bytes of the runs kernels (so_runs, kmp_runs); 0 = default
 *   6  SO: 0 so_runs (bank-private table, line fetch) / 1 so_scan (LDS tiles) / 2 so_runs64
 *      (shared table, 64-byte steps); SA: 3 = its own AND form (default: the complemented, Shift-Or form);
 *      5 so_runs a byte per table lookup even on a text of at most four byte values (round 3: there it takes four)
 *   7  packed matcher: 0 default — v_mqsad_pk_u16_u8 references for m <= 7 and on texts of at most four byte values,
 *      dword compares otherwise, the neighbour lane's bytes by DPP (round 4) / 1 both loads cached / 3 one load +
 *      shuffle / 6 v_mqsad references at every length / 7 the second (cached) load instead of DPP / 8, 9 dword
 *      compares only
 * Settings whose kernels exist only in the A/B build (libsmartgpu_ab.so) are refused by the product library. */
int smartgpu_tune(int key, int value);

/* How many queued smartgpu_plan_launch() calls share one pass over the text: 0 = none (every launch is sent at
 * once), 2..8.  Returns the previous value, SMARTGPU_ERR_ARG for anything else.  Needs no device; what is pending
 * is sent first.  This is the narrow view of the setting of smartgpu_coalesce_wide(): a previous value above 8 is
 * returned as 8. */
int smartgpu_coalesce(int max_group);
/* The same setting up to 32: 0 or 2..32.  Returns the previous value, a value above 32 (smartgpu_coalesce_pass) as 32;
 * SMARTGPU_ERR_ARG for anything else.  A pass set through this call or smartgpu_coalesce() is sent when exactly that
 * many launches have gathered, or at the next call that sends what is pending, whichever comes first. */
int smartgpu_coalesce_wide(int max_group);
/* The same setting over its whole range: 0 or 2..96, the most patterns one hor_multi_scan takes.  Returns the previous
 * value as it was, SMARTGPU_ERR_ARG for anything else.  How many patterns a pass really takes also depends on their
 * length, because a pass carries the end of every pattern in its kernel arguments: 96 up to m = 16, 84 up to m = 32,
 * 63 up to m = 48, 50 up to m = 64, 42 beyond; a wider setting is clipped to that per length, not refused.  The
 * library starts with 96 (profiles/coalesce/RESULTS.md has the measurements). */
int smartgpu_coalesce_pass(int max_group);
/* LONG passes.  What the 96 / 84 / 63 / 50 / 42 above bound is the room in the kernel's arguments; a pass that carries
 * pointers only, and reads the ends of its patterns from their plans, takes 252 up to m = 16, 152 up to m = 32, 108 up
 * to m = 48, 84 up to m = 64 and 68 beyond.  Under the widest setting (96) a key that reaches the width above is still
 * sent at once, unless its range holds at least `min_range_bytes` start positions AND the previous pass over the same
 * text, range and length left because it was full, with nothing since that sent what was pending (a sync, a result, a
 * mark, a setting): then the launches arrive faster than the GPU reads the text, and the key gathers up to the long
 * width, or until the next such call, and saves a read of the text.  The same holds for the first pass of a key whose
 * launches came so fast (the host clock at its first launch and at the one that fills it) that gathering on idles the
 * GPU for less than a pass over the range takes, where that is 10 us or more.  -1: no long passes; 0: any range.  Returns the
 * previous value (-1 or more), SMARTGPU_ERR_ARG for a value below -1.  Needs no device; what is pending is sent first.
 * The library starts with 64 MiB (profiles/coalesce/RESULTS.md has the measurements). */
long long smartgpu_coalesce_long(long long min_range_bytes);
/* Of the launches on `device` that could share a pass: how many were seen, and how many kernels were sent for them
 * (equal when nothing was coalesced).  Either pointer may be NULL. */
int smartgpu_coalesce_stats(int device, uint64_t *launches, uint64_t *passes);
/* How many launches on `device` rode in a pass that was gathering beside them (smartgpu_plan_launch: a pattern whose
 * symbols repeat, over a text whose symbols do not).  They are not among the `launches` above, and a pass that carries
 * them is counted in `passes` once, as any kernel sent; a key is sent when its other launches reach the coalesce setting
 * or when launches and riders together fill the room a pass of their length has. */
int smartgpu_coalesce_riders(int device, uint64_t *riders);
/* SAMPLED passes.  A text created by smartgpu_text_upload(), _upload_tiled() or _generate() with at least `min_bytes`
 * bytes gets a SAMPLE: the 4 bytes at every 28th position, n / 7 bytes of device memory, written once behind the
 * alphabet pass and freed with the text.  -1: no text created from now on gets one; 0: every text does.  Returns the
 * previous value, SMARTGPU_ERR_ARG for a value below -1; texts that exist keep what they have.  A failed allocation of
 * the sample is no error: the text has none.  The library starts with 64 MiB. */
long long smartgpu_text_sampling(long long min_bytes);
int smartgpu_text_has_sample(const smartgpu_text *t);
/* A shared pass over a text that has a sample, for patterns of 31 bytes or more, reads the sample instead of the text
 * (hor_sample_scan): every window that long holds one sampled 4-byte gram whole, so the pass filters on the sample
 * and compares, in the text, only the windows whose gram equals a gram of one of its patterns.  Counts are exact.
 * Such a pass takes 84 patterns at every length, 252 as a long pass.  on = 0 sends every pass to hor_multi_scan as
 * before; returns the previous value.  Needs no device; what is pending is sent first.  The library starts with 1. */
int smartgpu_coalesce_sample(int on);
/* How many passes on `device` went to hor_sample_scan (they are among the `passes` of smartgpu_coalesce_stats). */
int smartgpu_coalesce_sampled(int device, uint64_t *passes);
/* The workgroups of a sampled pass: 0 = one per compute unit (the default), 1..65536 = that many, fewer where the
 * range has fewer rows of 4096 samples.  For measurements and tests; returns the previous value. */
int smartgpu_coalesce_sample_grid(int workgroups);

/* Host-side preprocessing exposed for tests (same tables the kernels stage in
 * LDS): writes up to `cap` 32-bit entries, returns the number written or <0.
 *   which: 0 Horspool bad-char (256)      hor.c:26-30 / bm.c:27-33
 *          1 BM good-suffix (m)           bm.c:36-66
 *          2 KMP failure function (m+1)   kmp.c:27-41
 *          3 Shift-Or masks (256)         so.c:27-38   (32-bit words, prefix of 32 for m>32)
 *          4 BNDM masks (256)             bndm.c:35-40 (same)
 *          5 KMP transition table ((m+1)*256, m <= 255): the failure links of kmp.c:27-41
 *            expanded into delta[state][byte]; state m = an occurrence ends here
 *          6 the same over the pattern's own alphabet: k1, colmap[256], table[(m+1)*k1]
 *          7 Shift-And masks S[256] (sa.c:27-34), 8 Quick Search shifts qsBc[256] (qs.c:27-31),
 *          9 kmp_runs' tables as the kernel holds them in LDS (bytes; the last 272: Q and thr),
 *          10 the two-bit codes of the byte values of P taken as a SET (what the runs kernels use on a text of at most
 *            four byte values): shift, symtab — code (c >> shift) & 3, byte `code` of symtab = the member with that code
 *            (a non-member with that code if none); 0 entries when there are more than four or no shift separates them,
 *          13/15/18 HASH3/5/8 shifts[256] followed by the shift after a candidate (hash3.c:36-56)   */
int smartgpu_build_table(int which, const uint8_t *P, uint32_t m, int32_t *out, uint32_t cap);

/* ---- packed texts: at most four distinct byte values, held as bit planes -------------------------------------
 * A text of n symbols over k <= 4 distinct byte values, resident in one GPU's HBM as BIT PLANES: plane b holds bit b of
 * every symbol's code, 32 symbols per dword (symbol i = bit i % 32 of dword i / 32).  Codes are the ranks of the byte
 * values that occur, ascending; k <= 2 keeps ONE plane, k = 3, 4 two.  The same symbols in an eighth / a quarter of the
 * bytes of the byte text, counted by planes_scan (smart_amd/csrc/k_planes.hip) — three vector instructions per pattern
 * symbol for 32 start positions at once.  None of the reference's search() functions reads such a text, so there is no
 * algorithm id: the contract is the count BY DEFINITION (src/algos/bf.c:25-39), overlapping occurrences counted, for
 * every 1 <= m <= SMARTGPU_XSIZE; none of the reference's documented deviations applies.
 * Occurrence POSITIONS come from the same matcher with an output stage (planes_find; smartgpu_pfind64 and
 * smartgpu_pfind_batch64 below), so a packed text needs no byte copy beside it for smartgpu_find64.
 * Measured on an MI355X (profiles/packed/RESULTS.md), symbols per second against the byte text's best of SO / BNDM / HOR,
 * m = 2 .. 4096: 8 Gi symbols of four values 2.9-3.6 x, 1 Gi of four values 2.7-3.9 x, 1 Gi of two values 2.9-6.7 x. */
typedef struct smartgpu_ptext smartgpu_ptext;
/* Pure arithmetic, no device: planes (1 or 2) and HBM bytes per plane, pads excluded, for n symbols of `nvalues` distinct
 * values: 4 * ceil(n / 32).  SMARTGPU_ERR_ARG for nvalues < 1 or > 4.  Either pointer may be NULL. */
int smartgpu_ptext_layout(uint64_t n, int nvalues, int *planes, uint64_t *plane_bytes);
/* Packs a resident text ON THE DEVICE (one pass over it, planes_pack).  NULL, and a message that names the number of
 * values in smartgpu_last_error(), when the text holds more than four distinct values.  The byte text stays valid and
 * independent. */
smartgpu_ptext *smartgpu_ptext_pack(const smartgpu_text *t);
/* host bytes -> packed, through smartgpu_text_upload and the pack kernel; the byte copy is released */
smartgpu_ptext *smartgpu_ptext_upload(const void *host, uint64_t n, int device);
void smartgpu_ptext_free(smartgpu_ptext *t);
uint64_t smartgpu_ptext_length(const smartgpu_ptext *t); /* symbols */
int smartgpu_ptext_device(const smartgpu_ptext *t);
int smartgpu_ptext_planes(const smartgpu_ptext *t);      /* 1 or 2 (3: a text of the ...8 constructors below) */
uint64_t smartgpu_ptext_bytes(const smartgpu_ptext *t);  /* HBM bytes of the planes, pads excluded */
/* returns k, the number of distinct values; values[code] = the byte value of each code, ascending */
int smartgpu_ptext_symbols(const smartgpu_ptext *t, uint8_t values[4]);
/* symbols [off, off+len) unpacked to bytes on the host */
int smartgpu_ptext_read(const smartgpu_ptext *t, uint64_t off, uint64_t len, void *host);
/* Occurrences of P[0..m) with start s in [off, off+n-m]: the range convention, count width, pre_ms / run_ms meaning and
 * error codes of smartgpu_search64 (m = 0 or m > SMARTGPU_XSIZE: SMARTGPU_ERR_ARG; m > n: count 0).  A pattern byte the
 * text does not hold: count 0, no launch.  Not slower than the byte text in any measured cell (rand4 and rand2, m = 2 ..
 * 4096, profiles/packed/RESULTS.md); texts with long partial matches were not measured for speed. */
int smartgpu_psearch64(const uint8_t *P, uint32_t m, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                       uint64_t *count, double *pre_ms, double *run_ms);
/* K patterns of m bytes: K launches back to back on the device's stream, ONE read-back (the shape of
 * smartgpu_search_batch64 without its one-grid form).  *batch_ms (or NULL): first launch to the counts on the host. */
int smartgpu_psearch_batch64(const uint8_t *const *P, uint32_t m, uint32_t K, const smartgpu_ptext *text,
                             uint64_t off, uint64_t n, uint64_t *counts, double *batch_ms);
/* Occurrence positions on a packed text: every s in [off, off+n-m] with symbols [s, s+m) == P, ascending, relative to
 * symbol 0 of the text — the conventions of smartgpu_find64, the argument checks of smartgpu_psearch64.  *count always
 * receives the number of occurrences.  SMARTGPU_OK when count <= cap: the list is complete.  SMARTGPU_ERR_NOMEM when it is
 * not (the message names both numbers; the contents of positions are then unspecified).  cap == 0 with positions == NULL
 * is a count.  count == NULL, or positions == NULL with cap > 0: SMARTGPU_ERR_ARG.  m > n, or a pattern byte the text does
 * not hold: count 0, no launch.  The device buffer of up to 8 Mi positions is the device's own and kept between calls; when
 * the device has no memory for min(cap, start positions) entries the call counts and reports SMARTGPU_ERR_NOMEM. */
int smartgpu_pfind64(const uint8_t *P, uint32_t m, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                     uint64_t *positions, uint64_t cap, uint64_t *count);
/* K patterns of m symbols: the positions of pattern k are positions[starts[k] .. starts[k+1]), each slice ascending;
 * starts has K+1 entries, starts[0] = 0, starts[K] = the total.  Two passes over the planes: the counting batch
 * (smartgpu_psearch_batch64), then K finds back to back, each into its own slice, and ONE copy to the host.
 * starts[K] > cap: SMARTGPU_ERR_NOMEM with starts filled — every count and the room to allocate — and no find launched.
 * K is bounded as in smartgpu_psearch_batch64. */
int smartgpu_pfind_batch64(const uint8_t *const *P, uint32_t m, uint32_t K, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                           uint64_t *positions, uint64_t cap, uint64_t *starts);
/* SET patterns on a packed text: pattern position j accepts a set of the text's values instead of one (IUPAC motifs and
 * primers such as TATAWAW or GGNCC, restriction sites with N gaps).  The contract is the count by definition with
 * "T[s+j] == P[j]" replaced by "the code of T[s+j] is a member of sets[j]"; nothing in the reference does this.
 * sets[j], 0 <= j < m: bit c set = position j accepts the symbol with code c (values[c] of smartgpu_ptext_symbols).
 * One pass over the planes whatever the sets are (planes_sets_scan, planes_sets_find): a position costs the one
 * three-input bit operation per plane dword of an exact symbol, with the OR of its members' truth tables, and a position
 * that accepts every value of the text costs nothing.
 * The range convention, count width, times, cap / count / SMARTGPU_ERR_NOMEM behaviour and the order of the positions
 * (ascending, relative to symbol 0) are those of smartgpu_psearch64 / smartgpu_pfind64.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: sets == NULL, m = 0 or m > SMARTGPU_XSIZE, a NULL text,
 * a range outside the text, count == NULL, positions == NULL with cap > 0, and a set with a bit at or above the text's
 * number of values (bits 4..7 always are on one and two planes; the message names the position).
 * No launch: a position with the empty set (count 0, SMARTGPU_OK), m > n (count 0), a pattern of full sets (every start
 * position of the range; the find writes them when count <= cap).
 * MEASURED on an MI355X, 1 Gi symbols of rand4 and of rand2, m = 8 .. 256 (profiles/packed/RESULTS.md, "Set patterns"):
 * a singleton-set pattern is NOT at smartgpu_psearch64's speed, as the instruction count per position had suggested —
 * planes_sets_scan takes 1.45-1.63 x planes_scan's kernel time (1.26-1.45 x per call), outside the run-to-run spread in
 * every cell: the scalar switch per position and the larger loop body cost that much.  A motif with g = 1, 2, 3 full-set
 * positions in one call against its 4^g exact expansions through smartgpu_psearch_batch64 (rand4, m = 16): 2.1 / 7.6 /
 * 29.9 x faster, counts equal.  Two-member sets at the first eight positions (the early leave's worst case): 2.0-2.1 x
 * the exact pattern's call on rand4 from m = 16 on.  The rand2 planes are of Infinity-Cache size: possibly flattered.
 * NOT measured: the find form's speed, texts with long partial matches, texts beyond 1 Gi symbols. */
int smartgpu_psearch_sets64(const uint8_t *sets, uint32_t m, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                            uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_sets64(const uint8_t *sets, uint32_t m, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                          uint64_t *positions, uint64_t cap, uint64_t *count);
/* No device: IUPAC nucleotide letters -> sets over a text's values.  P[0..m): the letters A C G T U R Y S W K M B D H V N
 * in either case.  Value v of the text (values[0..nvalues), as smartgpu_ptext_symbols returns them) stands for base X when
 * it is the byte 'X' or 'x'; 'U' / 'u' count as T.  sets[j] = the OR over the text's values that position j's letter
 * accepts; it may be 0 (then the searches answer 0).  Any other byte in P: SMARTGPU_ERR_ARG, the message names position and
 * byte; nvalues outside 1..4 or a NULL pointer: SMARTGPU_ERR_ARG.  Nothing is written on refusal. */
int smartgpu_iupac_sets(const uint8_t values[4], int nvalues, const char *P, uint32_t m, uint8_t *sets);
/* MISMATCHES on a packed text: the occurrences of P with at most k mismatches ("where does this 20-mer occur with at most
 * two substitutions?").  Start position s (off <= s <= off + n - m) is an occurrence when its DISTANCE — the number of
 * j < m with T[s+j] != P[j], the Hamming distance over bytes — is at most k; nothing in the reference does this.
 * 0 <= k <= SMARTGPU_PMIS_MAX; k = 0 is smartgpu_psearch64 / smartgpu_pfind64.  k >= m is legal: every start position of
 * the range is an occurrence, its distance is still reported.  A pattern byte the text does NOT hold is a mismatch in every
 * window (the exact calls answer 0 for such a pattern; these calls do not): with u such bytes, u > k gives count 0 without
 * a launch, otherwise the kernels run with the budget k - u, do not compare those positions, and u is part of every
 * reported distance.  One pass over the planes whatever k is (planes_mis_scan, planes_mis_find): a bit-sliced counter
 * of 1 / 2 / 3 dwords per 32 start positions for a budget up to 1 / 3 / 7 and a sticky "over budget" dword.
 * The range convention, count width, times, cap / count / SMARTGPU_ERR_NOMEM behaviour and the order of the positions
 * (ascending, relative to symbol 0) are those of smartgpu_psearch_sets64 / smartgpu_pfind_sets64.  mismatches may be NULL;
 * otherwise it has cap entries and mismatches[i] receives the distance of positions[i].
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P == NULL, m = 0 or m > SMARTGPU_XSIZE,
 * k > SMARTGPU_PMIS_MAX, a NULL text, a range outside the text, count == NULL, positions == NULL with cap > 0.
 * No launch: m > n (count 0), more foreign bytes than k (count 0).
 * NOT offered: a batch call, k > 7, byte texts.  (Byte texts: smartgpu_search_mis64 below.  Set patterns with mismatches: smartgpu_psearch_sets_mis64 below; insertions
 * and deletions: smartgpu_psearch_edit64 below.)
 * MEASURED on an MI355X, 1 Gi symbols (profiles/packed/RESULTS.md, "Mismatches"): on rand4, m = 8 .. 256, planes_mis_scan takes
 * 1.22-1.26 / 1.25-1.94 / 1.34-2.11 / 1.55-3.56 x planes_scan's kernel time for k = 0 / 1 / 3 / 7 (per call 1.07-1.17 /
 * 1.07-1.62 / 1.13-1.76 / 1.24-2.76 x), outside the run-to-run spread in every cell.  m = 16: ONE k = 1 call is 14.8 x
 * faster than the 16 smartgpu_psearch_sets64 calls with one full-set position each that give the same answer (0.119 against
 * 1.755 ms, counting only, no host union), outside the spread; one k = 2 call 114 x faster than its 120 placements (a
 * sample timed and scaled).  smartgpu_pfind_mis64 (m = 20, k = 2): 1.26 x a one-N smartgpu_pfind_sets64.  Two-value texts
 * with k = 7 and m > 32: nearly every wave verifies, 5.9 x the exact call on rand2 (planes of Infinity-Cache size).
 * NOT measured: kUnroll, occupancy, the early leave's interval, texts beyond 1 Gi symbols. */
#define SMARTGPU_PMIS_MAX 7
int smartgpu_psearch_mis64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                           uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_mis64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                         uint64_t *positions, uint8_t *mismatches, uint64_t cap, uint64_t *count);
/* SET patterns with MISMATCHES on a packed text ("where does the degenerate primer GGNCCWRTATAWAW bind with at most two
 * mismatches?").  Start position s (off <= s <= off + n - m) is an occurrence when its DISTANCE — the number of j < m for
 * which the code of T[s+j] is NOT a member of sets[j] — is at most k; sets[j] as in smartgpu_psearch_sets64.  That is the
 * minimum over the pattern's exact expansions of the Hamming distance: a window may lie within k of several expansions, so
 * the counts of smartgpu_psearch_mis64 over the expansions overlap and cannot be added.  Nothing in the reference does this.
 * 0 <= k <= SMARTGPU_PMIS_MAX.  With k = 0 the answers are those of smartgpu_psearch_sets64 / smartgpu_pfind_sets64, with
 * singleton sets those of smartgpu_psearch_mis64 / smartgpu_pfind_mis64, distances included.  k >= m is legal: every start
 * position of the range is an occurrence, its distance is still reported.
 * A position with the FULL set (every value the text holds) is never a mismatch and costs the kernels no instruction.  A
 * position with the EMPTY set is a mismatch in every window (smartgpu_psearch_sets64 answers 0 for such a pattern; these
 * calls do NOT): with u such positions, u > k gives count 0 without a launch, otherwise the kernels run with the budget
 * k - u, do not compare those positions, and u is part of every reported distance.
 * One pass over the planes whatever the sets and k are (planes_sets_mis_scan, planes_sets_mis_find): smartgpu_psearch_mis64's
 * bit-sliced counter fed with the complement of the set's membership truth table — a set position costs what an exact
 * symbol costs there.
 * The range convention, count width, times, cap / count / SMARTGPU_ERR_NOMEM behaviour (cap == 0 with NULL buffers is a
 * count), mismatches == NULL and the order of the positions are those of smartgpu_psearch_mis64 / smartgpu_pfind_mis64.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: sets == NULL, k > SMARTGPU_PMIS_MAX, m = 0 or
 * m > SMARTGPU_XSIZE, a NULL text, a range outside the text, count == NULL, positions == NULL with cap > 0, and a set with a
 * bit at or above the text's number of values (bits 4..7 always are on one and two planes; the message names the position).
 * No launch: m > n (count 0), more empty sets than k (count 0).
 * NOT offered: a batch call, k > 7, byte texts.  (Byte texts: smartgpu_search_mis_classes64 below.  Insertions and deletions: smartgpu_psearch_sets_edit64 below.)
 * NOT measured: everything — no timing of these calls has been taken (tools/sets_mis_probe.py takes the three comparisons:
 * singleton sets against smartgpu_psearch_mis64, k = 0 against smartgpu_psearch_sets64, one find against the finds over
 * the pattern's exact expansions); the occupancy choices are smartgpu_psearch_mis64's, taken over unmeasured. */
int smartgpu_psearch_sets_mis64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                                uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_sets_mis64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                              uint64_t *positions, uint8_t *mismatches, uint64_t cap, uint64_t *count);
/* EDIT DISTANCE on a packed text: the occurrences of P within k unit-cost substitutions, INSERTIONS and DELETIONS ("where does
 * this primer bind with one base skipped?" — invisible to smartgpu_psearch_mis64 at any k).  Nothing in the reference does this.
 * For the range [off, off+n) and every off <= e < off+n, D(e) is the minimum over off <= s <= e+1 of the Levenshtein distance
 * between P and the symbols [s, e]; s = e+1 is the empty substring, at distance m.  That is the last row of Sellers' dynamic
 * programme on the range alone — D[0][*] = 0, D[i][before off] = i —: a match never reaches outside the range.  An
 * OCCURRENCE is an END position e with D(e) <= k.  It is reported as e, the index of the match's last symbol relative to
 * symbol 0 of the text, together with D(e); start positions and alignments come from smartgpu_palign_edit64.  With k = 0 the occurrences are exactly
 * smartgpu_pfind64's positions plus m - 1.
 * 1 <= m <= SMARTGPU_PEDIT_MAXM; 0 <= k <= SMARTGPU_PMIS_MAX.  k >= m is legal: every end position of the range is an
 * occurrence, its distance is still reported.  m > n is legal here, unlike the Hamming calls: a short range can match with
 * deletions; only n + k < m is "count 0, no launch".  A pattern byte the text does not hold accepts nothing (a substitution,
 * or a deletion, wherever it is aligned): these calls need no bookkeeping for it.
 * The sets calls take sets[j] as smartgpu_psearch_sets64 does, with "T[e'] == P[j]" replaced by "the code of T[e'] is a
 * member of sets[j]"; an empty set accepts nothing, as a foreign byte; a full set accepts everything.  With singleton sets
 * the answers are those of the byte-pattern calls.
 * One pass over the planes (planes_edit_scan, planes_edit_find; smart_amd/csrc/k_pedit.hip): Myers' bit-vector recurrence
 * in Hyyrö's search form, one text symbol per step and lane — a column depends on the one before it, so these kernels walk
 * the text per lane where every other plane kernel decides 32 positions per instruction.  A lane owns 128 consecutive end
 * positions and walks up to m + k symbols before them without counting: (128 + m + k) / 128 = 1.07 .. 1.55 symbols walked
 * per symbol of the range.  The recurrence consumes only the masks "which pattern positions accept code c", so a set pattern
 * costs the kernels what a byte pattern costs.
 * The count width, times, cap / count / SMARTGPU_ERR_NOMEM behaviour (cap == 0 with NULL buffers is a count), distances == NULL
 * and the order (ascending, relative to symbol 0) are those of smartgpu_psearch_mis64 / smartgpu_pfind_mis64, with ends[i] /
 * distances[i] in place of positions[i] / mismatches[i].
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P / sets == NULL, m = 0 or m > SMARTGPU_PEDIT_MAXM (the
 * message names the limit), k > SMARTGPU_PMIS_MAX, a NULL text, a range outside the text, count == NULL, ends == NULL with
 * cap > 0, and — the sets calls — a set with a bit at or above the text's number of values (the message names the position).
 * NOT offered: affine or weighted costs, a batch call, byte texts.  (Byte texts: smartgpu_search_edit64 below.  m > 64 and k > 7: smartgpu_psearch_editl64 below, up to
 * 256 symbols and 31 edits.  Start positions and alignments: smartgpu_palign_edit64 below.)
 * MEASURED on an MI355X, 1 Gi symbols, m = 8 .. 64, k = 0 .. 7 (profiles/packed/RESULTS.md, "Edit distance"; tools/edit_probe.py):
 * on rand4 planes_edit_scan takes 0.90-1.06 ms for m <= 32 (one dword per column: 1.0-1.2 T symbols/s) and 1.49-1.81 ms for
 * m = 33, 64 (two dwords: 0.59-0.72 T symbols/s), per call 0.94-1.11 / 1.46-1.77 ms; the time grows with the warm-up factor and
 * hardly with the number of occurrences.  That is 5.5-24.7 x planes_mis_scan's kernel time at the same m and k (per call 5.5-
 * 19.8 x), outside the run-to-run spread in every cell: the nearest question the library already answers, not the same one.
 * On rand2 0.61-0.73 / 1.15-1.41 ms (planes of Infinity-Cache size: possibly flattered).
 * NOT measured: the run of 128 positions per lane against a longer one, the occupancy and the grid (planes_scan's, taken over),
 * the find form's speed, texts beyond 1 Gi symbols. */
#define SMARTGPU_PEDIT_MAXM 64
int smartgpu_psearch_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                            uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                          uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
int smartgpu_psearch_sets_edit64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                                 uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_sets_edit64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                               uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
/* START POSITIONS and ALIGNMENTS of edit-distance occurrences: which interval of the text an end position e reported by
 * smartgpu_pfind_edit64 stands for, and which symbols were substituted, added or skipped.  For the range [off, off+n), the
 * pattern (bytes or sets) and an end position off <= e < off+n, with D(e) as smartgpu_psearch_edit64 defines it:
 * START.  s(e) is the LARGEST s in [off, e+1] with ed(P, T[s..e]) = D(e): the shortest nearest substring (s = e+1 is the
 * empty substring, at distance m).  It is unique, and it is what a backward walk from e meets first.
 * ALIGNMENT.  A sequence of L <= m + k operations in text order from s to e, two bits each:
 *   0 '=': the text symbol is accepted by the pattern position; consumes one of each;
 *   1 'X': a substitution; consumes one of each, the symbol is not accepted;
 *   2 'I': a text symbol with no pattern partner (an insertion: a text symbol added); consumes text only;
 *   3 'D': a pattern symbol with no text partner; consumes pattern only.
 * I and D are the PATTERN's edits: they are the opposite letters from SAM's CIGAR with the text as the reference.
 * Which optimal alignment is returned is fixed, on the suffix distances R[i][j] = ed(P[i..m), T[s+j..e]), J = e - s + 1:
 * start at (i, j) = (0, 0); until i == m and j == J take the first of these that applies:
 *   1. if i < m, j < J and R[i+1][j+1] + (accepted ? 0 : 1) == R[i][j]: '=' or 'X';
 *   2. else if i < m and R[i+1][j] + 1 == R[i][j]: 'D';
 *   3. else 'I'.
 * PACKING.  Three uint64_t per occurrence: operation t is in bits 2 * (t mod 32) of word t / 32, the top byte of the third
 * word (bits 56..63) holds L, every other unused bit is 0 (m + k <= 71 operations take 142 bits).
 * INPUT.  ends[0..count): end positions relative to symbol 0 of the text, as smartgpu_pfind_edit64 returns them for the same
 * P, m, k, off, n — but any e in [off, off+n) is legal, in any order, duplicates included; a subset of the find's list is fine.
 * OUTPUT.  starts[i] = s(ends[i]); distances[i] = D(ends[i]), computed, not taken on trust (no distances are passed in);
 * ops[3i .. 3i+3) the alignment.  distances and ops may be NULL; ops == NULL skips the traceback.
 * AN END THAT IS NO OCCURRENCE is decided exactly: the kernel walks min(m + k, e - off + 1) columns backward, whose minimum
 * is D(e) whenever D(e) <= k (a match within k has at most m + k symbols); a minimum above k means D(e) > k, and then
 * starts[i] = UINT64_MAX, distances[i] = 255, the three ops words are 0, and the call still returns SMARTGPU_OK.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: the refusals of smartgpu_pfind_edit64 (P / sets == NULL, m
 * outside [1, SMARTGPU_PEDIT_MAXM], k > SMARTGPU_PMIS_MAX, a NULL text, a range outside the text, a set with a bit at or above
 * the text's number of values), ends == NULL or starts == NULL with count > 0, and an ends[i] outside [off, off+n) (the
 * message names i and the value).  count == 0 is SMARTGPU_OK with no launch.  Lists longer than the device's find buffer
 * (8 Mi entries: 8 Mi occurrences without ops, 2 Mi with them) are worked through in pieces of that size.
 * One lane per occurrence (planes_edit_align; smart_amd/csrc/k_palign.hip): the recurrence of the edit calls in its DISTANCE
 * form over the reversed pattern, walking e, e-1, ...; with ops every column goes to LDS and the traceback reads cell values
 * back from the columns' bit vectors.
 * NOT offered: the longest start, all starts, all optimal alignments; m > 64, k > 7 (smartgpu_palign_editl64 below: up to 256
 * symbols and 31 edits, on the ends of smartgpu_pfind_editl64), affine costs, a kernel that finds and aligns in one pass.  (Byte
 * texts: smartgpu_align_edit64 below.)
 * MEASURED on an MI355X, 1 Gi symbols of rand4 with planted copies of the pattern, about 1 Mi occurrences (7 Mi for m = 20,
 * k = 7, which rand4 holds by itself), every end of the find aligned, ms per call by the host clock, the list's copy to the
 * device and the results' copy back included (profiles/packed/RESULTS.md, "Edit distance: starts and alignments";
 * tools/align_probe.py): m = 20 / 64, k = 2 / 7: without ops 1.85-1.91 ms per Mi occurrences (1.8-2.0 ns per occurrence),
 * which ADDS 19-31 % TO THE FIND that produced the ends (6.7-9.8 ms; 45 ms for the 7 Mi); with ops 4.3-4.7 ms (4.0-4.5 ns
 * per occurrence), 44-71 % of the find, 2.3-2.6 x the call without ops, outside the run-to-run spread in every cell.
 * NOT measured: the kernel's own time (no kernel trace: how a call divides between kernel and copies is not known), 64 / 32
 * occurrences per workgroup against other sizes, the uncoalesced text loads, texts beyond 1 Gi symbols, positions beyond
 * 2^32 (the tests' texts have at most 2^20 + 3 symbols). */
int smartgpu_palign_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                           const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
int smartgpu_palign_sets_edit64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                                const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
/* EDIT DISTANCE, LONG PATTERNS: smartgpu_psearch_edit64 / smartgpu_pfind_edit64 and their sets forms for 1 <= m <=
 * SMARTGPU_PEDITL_MAXM = 256 symbols and 0 <= k <= SMARTGPU_PEDITL_MAXK = 31 edits — a short read, an adapter followed by a
 * barcode, a capture probe.  The contract is that of those calls, word for word, with only the bounds widened: D(e) is the
 * last row of Sellers' programme on the range alone; an occurrence is an END position e with D(e) <= k; ends are ascending
 * and relative to symbol 0, distances[i] = D(ends[i]); m > n is legal, only n + k < m is "count 0, no launch"; k >= m is
 * legal; a foreign byte or an empty set accepts nothing, a full set everything; cap / count / SMARTGPU_ERR_NOMEM and
 * distances == NULL behave the same, cap == 0 with NULL buffers is a count.  Lengths up to 64 are legal here too: the answers
 * are those of the calls above, from a second, independent kernel.
 * flags: 0, or SMARTGPU_PEDITL_ALL_BLOCKS (bit 0): compute every block of every column, without the cut-off described below.
 * The answers are the same; the bit exists for the cross-check and the measurement.  Any other bit is SMARTGPU_ERR_ARG.
 * One pass over the planes (planes_editl_scan, planes_editl_find; smart_amd/csrc/k_peditl.hip): the recurrence of the calls
 * above in BLOCKS of 32 pattern rows with Ukkonen's cut-off — a block is stepped only while a value <= k can lie in it, so
 * on DNA-like text a long pattern at a small k costs little more than its first block.  The number of active blocks is
 * shared by the 64 lanes of a wave.  A lane owns 512 consecutive end positions and walks up to m + k <= 287 symbols before
 * them without counting.  The find's entries are sorted on the host.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P / sets == NULL, m = 0 or m > SMARTGPU_PEDITL_MAXM, k >
 * SMARTGPU_PEDITL_MAXK (the messages name the limits), a flags bit other than SMARTGPU_PEDITL_ALL_BLOCKS, a NULL text, a
 * range outside the text, count == NULL, ends == NULL with cap > 0, and — the sets calls — a set with a bit at or above the
 * text's number of values (the message names the position).
 * NOT offered: m > 256, k > 31, affine or weighted costs, a batch call, byte texts.
 * (Start positions and ALIGNMENTS of long patterns on a packed text: smartgpu_palign_editl64 below.)
 * MEASURED on an MI355X, 1 Gi symbols, m = 64, 65, 100, 150, 256, k = 0, 3, 7, 15, 31, the pattern cut from the text
 * (profiles/packed/RESULTS.md, "Edit distance: long patterns"; tools/editl_probe.py).  rand4, planes_editl_scan: 1.48-1.77 ms
 * for m <= 100 at k <= 7 (0.60-0.72 T symbols/s), 2.13-2.22 ms at m = 150, 2.51-2.59 ms at m = 256 (one active block: the
 * growth with m is the warm-up), 2.28-3.76 ms at k = 15 and 2.35-4.86 ms at k = 31 (two and three active blocks); per call
 * 1.50-4.85 ms.  THE CUT-OFF'S WORTH: with SMARTGPU_PEDITL_ALL_BLOCKS the same cells take 2.07-9.66 ms; all blocks / cut-off is
 * 3.6-3.7 at m = 256, k <= 7 (the CPU counts 1.00 of 8 blocks active), 2.0 at m = 256, k = 31, 1.36-1.40 at m = 64, k <= 7, outside
 * the run-to-run spread in every cell; where every block is active anyway the cut-off form is the SLOWER one, by 3-7 % (m = 64
 * at k = 15 and 31, m = 65 at k = 31: its votes and branches buy nothing there).  AGAINST smartgpu_psearch_edit64 at m = 64,
 * k = 0, 3, 7, same pattern: 0.86-0.88 x its kernel time on rand4 (the longer run walks 1.13-1.14 symbols per owned one where
 * that kernel walks 1.50-1.55).  rand2 (planes of Infinity-Cache size: possibly flattered): 1.24-5.27 ms with the cut-off,
 * 1.61-7.18 ms with all blocks; 0.93 / 1.06 / 1.33 x smartgpu_psearch_edit64's kernel at m = 64, k = 0 / 3 / 7 — two values
 * keep the second block active from k = 7 on.
 * NOT measured: other run lengths, the occupancy, the number of active blocks on the device (the figures are the CPU's), the
 * find form's speed and the host ordering's share in it, texts beyond 1 Gi symbols. */
#define SMARTGPU_PEDITL_MAXM 256
#define SMARTGPU_PEDITL_MAXK 31
#define SMARTGPU_PEDITL_ALL_BLOCKS 1u   /* flags bit 0 */
int smartgpu_psearch_editl64(const uint8_t *P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext *text,
                             uint64_t off, uint64_t n, uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_editl64(const uint8_t *P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext *text,
                           uint64_t off, uint64_t n, uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
int smartgpu_psearch_sets_editl64(const uint8_t *sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext *text,
                                  uint64_t off, uint64_t n, uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_pfind_sets_editl64(const uint8_t *sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext *text,
                                uint64_t off, uint64_t n, uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
/* EDIT DISTANCE ON A BYTE TEXT: smartgpu_psearch_edit64 / smartgpu_pfind_edit64 asked of a smartgpu_text, whatever number of
 * byte values it holds — English, protein sequences, rand32 .. rand256, a log file ("where does `recieve` occur within one
 * edit?").  The contract is that of those calls with "byte" for "symbol": for the range [off, off+n) and every off <= e <
 * off+n, D(e) is the last row of Sellers' programme on the range alone — D[0][*] = 0, the column before off is D[i] = i —; an
 * OCCURRENCE is an END position e with D(e) <= k; ends are ascending and relative to text byte 0, distances[i] = D(ends[i]).
 * 1 <= m <= SMARTGPU_EDIT_MAXM, 0 <= k <= SMARTGPU_PMIS_MAX.  k >= m is legal: every end of the range is an occurrence and its
 * distance is still reported.  m > n is legal; only n + k < m is "count 0, no launch".  cap / count / SMARTGPU_ERR_NOMEM,
 * cap == 0 with NULL buffers as a count, distances == NULL and the meaning of pre_ms / run_ms are those of the packed calls
 * (pre_ms holds the masks' construction and staging).  A pattern byte the text does not hold needs no bookkeeping: it has a bit
 * in no mask that a text byte selects.  With k = 0 the ends are smartgpu_find64's positions plus m - 1.
 * CLASSES: position j accepts a SET of byte values, a 256-bit row: classes[32 * j + v / 8] bit v % 8 set means it accepts byte
 * v (32 * m bytes in all) — case-insensitive search, the protein codes B, Z and X.  An empty row accepts nothing, a full row
 * everything.  With one bit per row the answers are those of the byte-pattern calls.
 * One pass over the text (text_edit_scan, text_edit_find; smart_amd/csrc/k_tedit.hip): Myers' bit-vector recurrence in Hyyrö's
 * search form, one byte per step and lane.  The pattern is 256 masks, one per byte value (1 or 2 KiB, built on the host, read
 * from LDS by the kernels: they do not know classes from bytes); a workgroup brings 32 KiB of text into LDS with coalesced
 * loads and every lane walks its 128 end positions, and up to m + k bytes before them without counting, out of LDS.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P / classes == NULL, m outside [1, SMARTGPU_EDIT_MAXM] (the
 * message names the limit), k > SMARTGPU_PMIS_MAX, a NULL text, a range outside the text, count == NULL, ends == NULL with
 * cap > 0.  The calls are synchronous: launches pending in the coalescing queue are sent first, and they never enter it.
 * NOT offered: m > 64 and k > 7 (smartgpu_search_editl64 / smartgpu_find_editl64 below: up to 256 bytes and 31 edits), a batch
 * call, MultiText shards and the `smart` harness.
 * (Start positions and alignments: smartgpu_align_edit64 below.  Substitutions only, no shifts: smartgpu_search_mis64 below.)
 * MEASURED on an MI355X, 1 GiB texts, m = 8, 20, 32, 33, 64, k = 0, 3, 7 (profiles/tedit/RESULTS.md; tools/tedit_probe.py; kernel
 * times from a kernel trace, call times by the host clock, medians of 5 / 7, run-to-run spread at most 3 % of the median but for the
 * first cell measured — rand4, m = 8, k = 0: 5-8 % per call): on rand4, rand128 and the English corpus alike text_edit_scan takes 0.71-0.82 ms for m <= 32 (one dword per column:
 * 1.31-1.52 TB/s of text) and 1.20-1.44 ms for m = 33, 64 (two dwords: 0.75-0.90 TB/s), per call 0.72-0.83 / 1.22-1.46 ms; the time
 * grows with the warm-up factor (128 + m + k) / 128 and neither with the alphabet nor with the number of occurrences.
 * AGAINST smartgpu_psearch_edit64 on the same rand4 bytes packed, same P and k: 0.75-0.77 x its kernel time for m <= 32, 0.82-0.84 x
 * for m = 33, 64 (per call 0.75-0.77 / 0.82-0.84 x), outside the run-to-run spread in every cell: bytes cost nothing, the walk out
 * of LDS is faster than the walk out of two bit planes.  MASK-LOOKUP CONFLICTS: rand256 (all-distinct lookups) against a text of
 * one value (all-broadcast lookups) at the same m and k: 0.99-1.00 x, inside the spread in 14 of 15 cells (the kernel trace at
 * m = 20, k = 0: 0.99 x) — the data-dependent bank conflicts of the mask table are hidden behind the recurrence's arithmetic.
 * THE PADDED ROW (132 bytes in LDS per 128 of text) against an unpadded build, rand256, k = 3, per call: the unpadded one takes
 * 1.13-1.15 x for m <= 32 and 1.06 x for m = 33, 64, outside the spread in every cell.
 * NOT measured: the four workgroups per CU, the run of 128 positions per lane, a
 * double-buffered tile, the find form's speed, the classes calls (the same kernels, another table), texts beyond 1 GiB, hardware
 * counters (the conflicts above are inferred from times, not counted). */
#define SMARTGPU_EDIT_MAXM 64
int smartgpu_search_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                           uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                         uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
int smartgpu_search_edit_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                   uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_edit_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                 uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
/* EDIT DISTANCE ON A BYTE TEXT, LONG PATTERNS: smartgpu_search_edit64 / smartgpu_find_edit64 and their classes forms for
 * 1 <= m <= SMARTGPU_EDITL_MAXM = 256 bytes and 0 <= k <= SMARTGPU_EDITL_MAXK = 31 edits — a sentence or a log line with typos,
 * a protein domain of 100-150 residues, a 120-byte record, an English phrase at an error rate of 5-10 %.  The contract is that
 * of those calls, word for word, with only the bounds widened: the calls count and list END positions e in [off, off+n) with
 * D(e) <= k, D the last row of Sellers' programme on the range alone; ends are ascending and relative to text byte 0,
 * distances[i] = D(ends[i]); m > n is legal, only n + k < m is "count 0, no launch"; k >= m is legal; a byte the pattern does
 * not hold or an empty row accepts nothing, a full row everything; cap / count / SMARTGPU_ERR_NOMEM and distances == NULL
 * behave the same, cap == 0 with NULL buffers is a count.  classes: 32 bytes per position, smartgpu_search_edit_classes64's
 * rows.  Lengths up to 64 and k up to 7 are legal here too: the answers are those of the calls above, from a second,
 * independent kernel.
 * flags: 0, or SMARTGPU_EDITL_ALL_BLOCKS (bit 0): compute every block of every column, without the cut-off.  The answers are the
 * same; the bit exists for the cross-check and the measurement.  Any other bit is SMARTGPU_ERR_ARG.
 * One pass over the text (text_editl_scan, text_editl_find; smart_amd/csrc/k_teditl.hip): the recurrence of
 * smartgpu_psearch_editl64 — BLOCKS of 32 pattern rows with Ukkonen's cut-off, the number of active blocks shared by the 64
 * lanes of a wave — fed as smartgpu_search_edit64's kernels are fed: the pattern is 256 masks of 2, 4 or 8 dwords in LDS, one
 * dword read per active block, and the text comes into LDS by coalesced loads.  A lane owns 512 consecutive end positions and
 * walks them, and up to m + k <= 287 bytes before them without counting, in pieces of 128 bytes.  The find's entries are sorted
 * on the host.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P / classes == NULL, m outside [1, SMARTGPU_EDITL_MAXM], k >
 * SMARTGPU_EDITL_MAXK (the messages name the limits), a flags bit other than SMARTGPU_EDITL_ALL_BLOCKS, a NULL text, a range
 * outside the text, count == NULL, ends == NULL with cap > 0.  The calls are synchronous: launches pending in the coalescing
 * queue are sent first, and they never enter it.
 * NOT offered: m > 256, k > 31, a batch call, MultiText shards, the `smart` harness.
 * (Start positions and ALIGNMENTS of long patterns on a byte text: smartgpu_align_editl64 below.)
 * MEASURED on an MI355X, 1 GiB of rand128, English and rand4, m = 64, 65, 100, 150, 256, k = 0, 3, 7, 15, 31, the pattern cut
 * from the text (profiles/tedit/RESULTS.md, "Long patterns"; tools/teditl_probe.py; kernel times from a kernel trace taken in a
 * run of its own, medians of 5, run-to-run spread at most 2 % of the median; call times by the host clock, medians of 7, spread
 * at most 4 %).  text_editl_scan at k <= 7, on the three texts alike: 1.59-1.68 ms at m = 64 (0.64-0.68 TB/s of text), 1.77-1.99 ms
 * at m = 65, 100, 2.73-2.89 ms at m = 150, 3.15-3.42 ms at m = 256; at k = 15 1.66-3.51 ms on rand128 and English and 2.29-4.47 ms
 * on rand4 (four values keep the second block active), at k = 31 2.35-5.19 ms; per call 1.63-5.20 ms.  THE CUT-OFF'S WORTH: with
 * SMARTGPU_EDITL_ALL_BLOCKS the same cells take 1.94-7.96 ms; all blocks / cut-off is 2.26-2.45 at m = 256, k <= 7 (the packed
 * kernel's 3.6 is not reached), 1.71-1.82 at m = 150, 1.65-1.75 at m = 100, 1.39-1.48 at m = 65, 1.17-1.24 at m = 64, 1.53-1.74 at
 * m = 256, k = 31, outside the spread in all of these; where every block is active anyway the cut-off form is the SLOWER one: all
 * blocks / cut-off is 0.85-0.87 (m = 64 at k = 31, and at k = 15 on rand4) and 0.89-0.99 (m = 65 at k = 31); inside the spread: m = 65 at k = 31 on rand128,
 * m = 65 at k = 15 on rand4, per call also m = 65, k = 31 on English and m = 100, k = 31 on rand4.  AGAINST smartgpu_search_edit64
 * (text_edit_scan, unchanged) at m = 64, k = 0, 3, 7, same pattern: 1.12-1.16 x its kernel time on all three texts, outside the
 * spread: on the length both can do the two-dword kernel is the faster one.  AGAINST smartgpu_psearch_editl64 (planes_editl_scan)
 * on the same rand4 bytes packed, same P and k: 1.08-1.12 x its kernel time for m <= 100 at k <= 7, 1.27-1.29 x for m = 150, 256
 * at k <= 7, 1.06-1.21 x at k = 15 (m >= 65), 1.08 x at m >= 150, k = 31, 0.95-0.96 x at m = 65, 100, k = 31, 1.00 x (inside the
 * spread) at m = 64, k = 15, 31: bytes cost 8-29 % here, where the warm-up pieces are parked whole for every lane.  The step from
 * m = 100 to m = 150 (1.45 x, for 1.08 x the bytes walked) coincides with the 8-dword kernel, which runs 3 workgroups per CU
 * instead of 4; the two were not separated.
 * NOT measured: the occupancy choice (4 / 4 / 3 workgroups per CU is what the LDS holds), other run and piece lengths, a
 * prefetch of the next piece, the find form's speed and the host ordering's share in it, the classes calls, texts beyond 1 GiB. */
#define SMARTGPU_EDITL_MAXM 256
#define SMARTGPU_EDITL_MAXK 31
#define SMARTGPU_EDITL_ALL_BLOCKS 1u   /* flags bit 0 */
int smartgpu_search_editl64(const uint8_t *P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text *text,
                            uint64_t off, uint64_t n, uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_editl64(const uint8_t *P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text *text,
                          uint64_t off, uint64_t n, uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
int smartgpu_search_editl_classes64(const uint8_t *classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text *text,
                                    uint64_t off, uint64_t n, uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_editl_classes64(const uint8_t *classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text *text,
                                  uint64_t off, uint64_t n, uint64_t *ends, uint8_t *distances, uint64_t cap, uint64_t *count);
/* START POSITIONS and ALIGNMENTS on a byte text: smartgpu_palign_edit64 / smartgpu_palign_sets_edit64 asked of a
 * smartgpu_text — which bytes an end position e reported by smartgpu_find_edit64 / smartgpu_find_edit_classes64 stands for,
 * and which of them were substituted, added or skipped.  The contract is that of smartgpu_palign_edit64, word for word,
 * with "byte" for "symbol" and D(e) as smartgpu_search_edit64 defines it: START, ALIGNMENT (the four operations and the
 * fixed choice among optimal alignments) and PACKING are stated there and hold here unchanged.
 * INPUT.  ends[0..count): end positions relative to text byte 0, as the find returns them for the same pattern, m, k, off,
 * n — but any e in [off, off+n) is legal, in any order, duplicates included.
 * OUTPUT.  starts[i] = s(ends[i]), distances[i] = D(ends[i]) (computed, not taken on trust), ops[3i .. 3i+3) the alignment;
 * distances and ops may be NULL, ops == NULL skips the traceback.  An end with D(e) > k is decided exactly by
 * min(m + k, e - off + 1) columns: starts[i] = UINT64_MAX, distances[i] = 255, three zero words, and the call still returns
 * SMARTGPU_OK.
 * CLASSES: the 32 * m bytes of smartgpu_search_edit_classes64; an empty row accepts nothing, a full row everything.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: the refusals of smartgpu_find_edit64 (P / classes == NULL,
 * m outside [1, SMARTGPU_EDIT_MAXM], k > SMARTGPU_PMIS_MAX, a NULL text — with count == 0 too —, a range outside the text),
 * ends == NULL or starts == NULL with count > 0, and an ends[i] outside [off, off+n) (the message names i and the value).
 * count == 0 with a valid text is SMARTGPU_OK with no launch.  Lists longer than the device's find buffer go through in
 * pieces, as for the packed calls.  The calls are synchronous: launches pending in the coalescing queue are sent first,
 * and they never enter it.
 * One lane per occurrence (text_edit_align; smart_amd/csrc/k_talign.hip): the recurrence in its DISTANCE form over the
 * reversed pattern's 256 masks, which the workgroup copies to LDS (one barrier); a lane parks the 11 or 19 aligned dwords
 * that hold its at most m + k <= 71 bytes in LDS and walks e, e-1, ...; with ops every column goes to LDS as well and the
 * traceback reads cell values back from the columns' bit vectors.
 * NOT offered: the longest start, all starts or all optimal alignments of a byte text; m > 64, k > 7 (smartgpu_align_editl64 below); a kernel that finds
 * and aligns in one pass; a batch call; MultiText shards; the `smart` harness; three-plane texts.
 * MEASURED on an MI355X, 1 GiB of rand128, English and rand4 with planted copies of the pattern, about 1 Mi occurrences (9.5 Mi
 * for rand4 at m = 20, k = 7, which it holds by itself), every end of the find aligned, ms per call by the host clock, the
 * list's copy to the device and the results' copy back included, medians of 7 (profiles/tedit/RESULTS.md, "Starts and
 * alignments"; tools/talign_probe.py): m = 20 / 64, k = 2 / 7, on all three texts alike: without ops 1.6-2.1 ms per call
 * (1.5-1.9 ns per occurrence), which ADDS 25-32 % TO THE FIND that produced the ends (5.3-6.6 ms; 56 ms for the 9.5 Mi); with ops
 * 3.0-4.5 ms (2.9-4.3 ns per occurrence), 48-77 % of the find, 1.8-2.7 x the call without ops, outside the run-to-run spread
 * in every cell.  AGAINST smartgpu_palign_edit64 on the same rand4 bytes packed, same P, k and ends (identical answers):
 * 0.97-1.00 x without ops, 1.00-1.10 x with ops, INSIDE the run-to-run spread in every cell.
 * NOT measured: the kernel's own time (no kernel trace: how a call divides between kernel and copies is not known), the LDS
 * copy of the table against reads from the arena, 64 / 32 occurrences per workgroup against other sizes, the uncoalesced
 * window loads, the classes calls (the same kernels, another table), texts beyond 1 GiB (the at-size test checks answers
 * beyond 2^32, not times). */
int smartgpu_align_edit64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                          const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
int smartgpu_align_edit_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                  const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
/* START POSITIONS and ALIGNMENTS of LONG patterns on a byte text: smartgpu_align_edit64 for 1 <= m <= SMARTGPU_EDITL_MAXM =
 * 256 bytes and 0 <= k <= SMARTGPU_EDITL_MAXK = 31 edits — which bytes an end position e reported by smartgpu_find_editl64 /
 * smartgpu_find_editl_classes64 stands for (an interval of m - k to m + k bytes that the end and the distance do not
 * identify), and which of them were substituted, added or skipped.  The contract is that of smartgpu_align_edit64, word for
 * word: the LARGEST nearest start, D(e) computed and not taken on trust, the same four operations, the same fixed choice
 * among optimal alignments (the diagonal first, then 'D', then 'I'), any e in [off, off+n) in any order with duplicates, the
 * sentinels for D(e) > k decided exactly from min(m + k, e - off + 1) columns, start = e + 1 (the empty match, L = m
 * deletions) when m <= k.  Lengths <= 64 with k <= 7 are legal too and give the starts, distances and operations of
 * smartgpu_align_edit64, from an independent kernel.  Three things differ:
 * BOUNDS: as above, and the messages name them.
 * PACKING: ops has SMARTGPU_ALIGNL_OPS_WORDS = 10 words per entry, because an alignment has at most m + k = 287 operations:
 * operation t in bits 2 * (t mod 32) of word t / 32, words 0 .. 8; word 9 holds the length L; every other bit is 0.  An end
 * that is no occurrence gets ten zero words.  (The two-bit codes are smartgpu_palign_edit64's.)
 * DISTANCES: distances[i] <= 31, or 255 for the sentinel (starts[i] = UINT64_MAX).
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written, in smartgpu_align_edit64's order: ends == NULL or starts ==
 * NULL with count > 0, P / classes == NULL, m outside [1, SMARTGPU_EDITL_MAXM], k > SMARTGPU_EDITL_MAXK, a NULL text — with
 * count == 0 too —, a range outside the text, and an ends[i] outside [off, off+n) (the message names i and the value).
 * count == 0 with a valid text is SMARTGPU_OK with no launch.  Lists longer than the device's find buffer go through in
 * pieces (a piece: the buffer's entries / 11 occurrences with ops).  The calls are synchronous: launches pending in the
 * coalescing queue are sent first, and they never enter it.
 * One WAVE per occurrence, one LANE per diagonal (text_editl_align; smart_amd/csrc/k_talignl.hip, alignl_band.hpp): a cost
 * <= k <= 31 never leaves the 63 diagonals |i - j| <= k, which fit a 64-lane wave.  The wave parks the 73 aligned dwords that
 * hold its at most 287 bytes in LDS, sweeps the anti-diagonals of the reversed matrix with two DPP wave shifts and one read
 * of the reversed pattern's 256 masks (in LDS, one barrier) per step, and reduces row m to (D(e), J).  With ops every cell's
 * two-bit decision goes to LDS, 17 dwords per lane, and a wave-uniform walk reads them back; no bit-vector column is stored.
 * NOT offered: the longest start, all starts or all optimal alignments; m > 256, k > 31; a kernel that finds and aligns in one
 * pass; a batch call; MultiText shards; the `smart` harness.  (Packed texts: smartgpu_palign_editl64 below.)
 * MEASURED on an MI355X, 1 GiB of rand128, English and rand4 with planted copies of the pattern, about 1 Mi occurrences, m = 64,
 * 100, 150, 256, k = 7, 15, 31, every end of smartgpu_find_editl64 aligned, ms per call by the host clock, the list's copy to
 * the device and the results' copy back included, medians of 7, run-to-run spread at most 5 % of the median
 * (profiles/tedit/RESULTS.md, "Long patterns: starts and alignments"; tools/talignl_probe.py), on the three texts alike: without
 * ops 9.5-11.8 ms at m = 64, 13.8-15.8 ms at m = 100, 19.8-21.8 ms at m = 150, 32.1-34.4 ms at m = 256 (9-33 ns per occurrence;
 * the time follows 2 m + k, the number of anti-diagonals), which is 34-123 % OF THE FIND that produced the ends (23.7-33.0 ms);
 * with ops 23.0-69.2 ms (22-65 ns per occurrence), 83-244 % of the find, 1.99-2.55 x the call without ops, outside the
 * spread in every cell.  AGAINST smartgpu_align_edit64 (text_edit_align, unchanged) at m = 64, k = 7 on the same ends
 * (identical starts, distances and operations): 5.0-5.3 x without ops, 4.8-5.2 x with ops: on the lengths both can do the
 * short call is the one to use.  rand4 at m = 64, k = 31 holds 160 Mi occurrences by itself and was not measured.  The
 * follow-up for the call without ops is a lane-per-occurrence bit-parallel walk (edit_block.hpp's recurrence in its
 * distance form, no decisions kept); it is not built.
 * NOT measured: the kernel's own time (no kernel trace: how a call divides between kernel and copies is not known), occupancy,
 * DPP against ds_bpermute for the neighbours' values, the serial traceback's latency, the classes calls (the same kernels,
 * another table), texts beyond 1 GiB (the at-size test checks answers beyond 2^32, not times). */
#define SMARTGPU_ALIGNL_OPS_WORDS 10
int smartgpu_align_editl64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                           const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
int smartgpu_align_editl_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                   const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
/* START POSITIONS and ALIGNMENTS of LONG patterns on a PACKED text: smartgpu_palign_edit64 for 1 <= m <= SMARTGPU_PEDITL_MAXM =
 * 256 symbols and 0 <= k <= SMARTGPU_PEDITL_MAXK = 31 edits — which symbols an end position e reported by smartgpu_pfind_editl64
 * / smartgpu_pfind_sets_editl64 stands for, and which of them were substituted, added or skipped, with no byte copy of the text
 * on the device.  The contract is that of smartgpu_palign_edit64 with the bounds, the packing and the distances of
 * smartgpu_align_editl64 above: the LARGEST nearest start, D(e) computed and not taken on trust, the same four operations, the
 * same fixed choice among optimal alignments (the diagonal first, then 'D', then 'I'), any e in [off, off+n) in any order with
 * duplicates, the sentinels for D(e) > k (starts[i] = UINT64_MAX, distances[i] = 255, ten zero words) decided exactly from
 * min(m + k, e - off + 1) columns, ops of SMARTGPU_ALIGNL_OPS_WORDS = 10 words per entry (operation t in bits 2 * (t mod 32) of
 * word t / 32, words 0 .. 8; word 9 holds L).  On the same bytes uploaded as a smartgpu_text, smartgpu_align_editl64 gives the
 * same starts, distances and ten words, bit for bit; for m <= 64 and k <= 7 smartgpu_palign_edit64 gives the same starts,
 * distances and operations.  A foreign byte or an empty set accepts nothing, a full set everything, as in the finds.
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written, in smartgpu_palign_edit64's order: ends == NULL or starts ==
 * NULL with count > 0, P / sets == NULL, m outside [1, SMARTGPU_PEDITL_MAXM], k > SMARTGPU_PEDITL_MAXK, a NULL text — with
 * count == 0 too —, a three-plane text, a range outside the text, a set with a bit at or above the text's number of values (the
 * message names the position), and an ends[i] outside [off, off+n) (the message names i and the value).  count == 0 with a
 * valid text is SMARTGPU_OK with no launch.  Lists longer than the device's find buffer go through in pieces (a piece: the
 * buffer's entries / 11 occurrences with ops).  The calls are synchronous: launches pending in the coalescing queue are sent
 * first, and they never enter it.
 * One WAVE per occurrence, one LANE per diagonal (planes_editl_align; smart_amd/csrc/k_palignl.hip, alignl_band.hpp): the
 * decomposition of text_editl_align, fed from bit planes.  The wave parks the 10 aligned dwords of each plane that hold its at
 * most 287 symbols in LDS (the byte kernel parks 73), takes a column's code from them by shift, and reads `miss` from the
 * reversed pattern's four masks of eight dwords, which travel as kernel arguments and lie in LDS (one barrier); the sweep of
 * the anti-diagonals with two DPP wave shifts, the decisions (17 dwords per lane), the reduction of row m and the wave-uniform
 * walk are the byte kernel's.
 * NOT offered: the longest start, all starts or all optimal alignments; three-plane texts; m > 256, k > 31; a kernel that finds
 * and aligns in one pass; a batch call.
 * NOT measured: everything — the call's time against smartgpu_align_editl64 on the same bytes unpacked, against
 * smartgpu_palign_edit64 at m = 64, k = 7, and as a share of the smartgpu_pfind_editl64 that produced the ends
 * (tools/palignl_probe.py takes the three; profiles/packed/RESULTS.md, "Long patterns: starts and alignments"), the kernel's own
 * time, occupancy. */
int smartgpu_palign_editl64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                            const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
int smartgpu_palign_sets_editl64(const uint8_t *sets, uint32_t m, uint32_t k, const smartgpu_ptext *text, uint64_t off, uint64_t n,
                                 const uint64_t *ends, uint64_t count, uint64_t *starts, uint8_t *distances, uint64_t *ops);
/* MISMATCHES ON A BYTE TEXT: smartgpu_psearch_mis64 / smartgpu_pfind_mis64 asked of a smartgpu_text, whatever number of byte
 * values it holds ("which fixed-width record fields, barcodes, motifs lie within k substitutions of this one, no shifts?").
 * The contract is that of those calls with "byte" for "symbol": a START position s, off <= s <= off + n - m, is an occurrence
 * when its DISTANCE — the number of j < m with T[s+j] != P[j] — is at most k.  Positions are ascending and relative to text
 * byte 0; mismatches may be NULL, otherwise mismatches[i] receives the distance of positions[i].
 * 1 <= m <= SMARTGPU_MIS_MAXM, 0 <= k <= SMARTGPU_PMIS_MAX.  With k = 0 the positions are smartgpu_find64's.  k >= m is legal:
 * every start position of the range is an occurrence, its distance is still reported.  m > n: count 0, no launch.  A pattern
 * byte the text does not hold needs no bookkeeping (the packed calls count such bytes on the host): it is a mismatch in every
 * window, through the masks.  cap / count / SMARTGPU_ERR_NOMEM, cap == 0 with NULL buffers as a count and the meaning of
 * pre_ms / run_ms are those of smartgpu_find_edit64 (pre_ms holds the masks' construction and staging).
 * CLASSES: the 32 * m bytes of smartgpu_search_edit_classes64 — classes[32 * j + v / 8] bit v % 8 set: position j accepts
 * byte v —; the distance is the number of j whose row does not accept T[s+j].  An empty row is a mismatch in every window, a
 * full row never is.  With one bit per row the answers are those of the byte-pattern calls.
 * These calls and smartgpu_search_edit64 answer different questions: that call reports END positions of matches of any length
 * from m - k to m + k and accepts insertions and deletions; at equal k every occurrence here has its end s + m - 1 among that
 * call's ends, not the other way round.
 * One pass over the text (text_mis_scan, text_mis_find; smart_amd/csrc/k_tmis.hip), in text_edit_scan's geometry: a workgroup
 * brings 32 KiB of text into LDS with coalesced loads, a lane walks the 128 windows that END in its run and the m - 1 bytes
 * before them.  The pattern is 256 masks "position j does not accept this byte" (1 or 2 KiB, built on the host, read from LDS);
 * per byte a lane shifts 1 / 2 / 3 bit-sliced counter dwords (k <= 1 / 3 / 7; twice as many for m > 32) and a sticky "over
 * budget" dword by one window, adds the byte's mask, and tests one bit: smartgpu_psearch_mis64's counter, turned so that
 * it moves with the text (smart_amd/csrc/tmis_host.hpp).
 * SMARTGPU_ERR_ARG, decided before any HIP call, nothing written: P / classes == NULL, m outside [1, SMARTGPU_MIS_MAXM] (the
 * message names the limit), k > SMARTGPU_PMIS_MAX, a NULL text, a range outside the text, count == NULL, positions == NULL with
 * cap > 0.  The calls are synchronous: launches pending in the coalescing queue are sent first, and they never enter it.
 * NOT offered: m > 64, k > 7, a batch call, MultiText shards, the `smart` harness, alignments (a Hamming alignment is the
 * window itself: T[s+j] against P[j]).
 * MEASURED on an MI355X, 1 GiB of rand4, rand128 and the English corpus, m = 8, 20, 32, 33, 64, k = 0, 1, 3, 7
 * (profiles/tedit/RESULTS.md, "Mismatches"; tools/tmis_probe.py; kernel times from a kernel trace, medians of 5, run-to-run
 * spread at most 5 % of the median; call times by the host clock, medians of 7): text_mis_scan takes 0.39-0.44 / 0.47-0.54 /
 * 0.56-0.64 ms for m <= 32 at k <= 1 / k = 3 / k = 7 (one, two, three counter dwords) and 0.59-0.70 / 0.78-0.93 / 0.98-1.17 ms for
 * m = 33, 64, the same on all three texts.  AGAINST text_edit_scan at the same text, P and k: 0.55-0.57 / 0.66-0.68 / 0.77-0.80 x
 * its kernel time for m <= 32 and 0.49-0.51 / 0.64-0.67 / 0.79-0.82 x for m = 33, 64, outside the spread in all 60 cells.
 * AGAINST smartgpu_psearch_mis64 on the same rand4 bytes packed: the planes win, text_mis_scan takes 3.5-10.7 x planes_mis_scan's
 * kernel time (3.3-8.2 x per call), outside the spread in every cell: a text of at most four values is worth packing.
 * smartgpu_find_mis64 at 2^20 occurrences (one per KiB): 4.9 ms per call against 0.60 ms (m = 20, k = 2) and 1.32 ms (m = 64,
 * k = 7) for the count, the list's copy, ordering and unpacking included.
 * NOT measured: the four workgroups per CU, the run of 128 positions per lane, the rolled walk against an unrolled one, the
 * compressed code object's load time, text_mis_find's kernel time, the classes calls (the same kernels, another table),
 * texts beyond 1 GiB, hardware counters. */
#define SMARTGPU_MIS_MAXM 64
int smartgpu_search_mis64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                          uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_mis64(const uint8_t *P, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                        uint64_t *positions, uint8_t *mismatches, uint64_t cap, uint64_t *count);
int smartgpu_search_mis_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                  uint64_t *count, double *pre_ms, double *run_ms);
int smartgpu_find_mis_classes64(const uint8_t *classes, uint32_t m, uint32_t k, const smartgpu_text *text, uint64_t off, uint64_t n,
                                uint64_t *positions, uint8_t *mismatches, uint64_t cap, uint64_t *count);
/* No device: the reverse complement of an IUPAC nucleotide pattern — a primer is searched on both strands.  P[0..m): the
 * letters smartgpu_iupac_sets accepts; out[j] = the complement of P[m-1-j]: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W and
 * N stay; U reads as T (its complement is A; no U is ever written).  Case is preserved.  out has m bytes (no terminator is
 * written) and may be P itself.  Any other byte: SMARTGPU_ERR_ARG, the message names position and byte, nothing is written. */
int smartgpu_iupac_revcomp(const char *P, uint32_t m, char *out);
/* smartgpu_probe_read_ms on the planes: the streaming-read time of the bytes a packed search reads (the plane roofline) */
int smartgpu_ptext_probe_read_ms(const smartgpu_ptext *t, int reps, double *ms_per_pass);

/* ---- packed texts of five to eight distinct byte values: THREE bit planes ---------------------------------------
 * An assembly with N (ACGNT: five values), a multi-record text with a separator, RNA/DNA mixes and reduced protein
 * alphabets do not fit two planes.  The ...8 constructors below pack such a text on three planes — plane b holds bit b of
 * the code, codes are the ranks of the byte values that occur, ascending, as above — at 3/8 of the byte text's HBM bytes.
 * For a text of at most FOUR values they produce exactly what smartgpu_ptext_pack / smartgpu_ptext_upload produce (one or
 * two planes, served by the same kernels afterwards).  More than eight values: NULL, and a message that names the number.
 * smartgpu_ptext_pack, smartgpu_ptext_upload, smartgpu_ptext_layout and smartgpu_iupac_sets are unchanged: they still
 * refuse more than four values.
 * The allocation is the two-plane one with a third plane, [front pad | plane 0 | back pad | plane 1 | back pad | plane 2 |
 * back pad], every plane 256-byte aligned, zero-filled before the pack: pad and tail bits look like code 0 and are never
 * counted.  smartgpu_ptext_planes answers 3, smartgpu_ptext_bytes 3 x the plane bytes; smartgpu_ptext_read and
 * smartgpu_ptext_probe_read_ms work on three planes.  smartgpu_ptext_symbols (four entries) answers SMARTGPU_ERR_ARG on a
 * three-plane text and names smartgpu_ptext_symbols8, which works on every packed text.
 *
 * OFFERED on a three-plane text, contract unchanged (ranges, count widths, times, cap / count / SMARTGPU_ERR_NOMEM,
 * ascending positions relative to symbol 0 with distances, the no-launch cases, the SMARTGPU_ERR_ARG cases decided before
 * any HIP call): smartgpu_psearch64, smartgpu_psearch_batch64, smartgpu_pfind64, smartgpu_pfind_batch64,
 * smartgpu_psearch_sets64, smartgpu_pfind_sets64, smartgpu_psearch_mis64, smartgpu_pfind_mis64, smartgpu_psearch_sets_mis64,
 * smartgpu_pfind_sets_mis64.  A set may carry bits up to nvalues - 1 <= 7; a bit at or above the text's number of values is
 * refused and the message names the position.  All ten go through ONE kernel pair, planes3_scan / planes3_find
 * (smart_amd/csrc/k_planes3.hip): an exact pattern travels as singleton sets; a set position costs three v_alignbit and
 * three three-input bit operations per 32 start positions (five instructions for a singleton, two or three for a set that
 * does not depend on plane 2, none for a position that accepts every value) where planes_scan takes three in all.
 * BATCH calls on a three-plane text: a pattern takes eight membership planes (4256 bytes) in the staging buffer and the
 * device arena instead of two code planes, so K <= 7884 per call (32 MiB / 4256); beyond: SMARTGPU_ERR_ARG before any HIP
 * call, the message names the bound.
 * NOT offered on a three-plane text: edit distance and alignments — the smartgpu_p*_edit64, smartgpu_p*_editl64 and
 * smartgpu_palign_* calls answer SMARTGPU_ERR_ARG before any HIP call, and the message says so.  (The obvious follow-up:
 * their match masks are per code already.)  Also not offered: more than eight values, byte texts.
 * MEASURED on an MI355X, 1 Gi symbols, m = 8 .. 256 (profiles/packed/RESULTS.md, "Three planes"; tools/wide_probe.py), no
 * threshold set in advance: exact count on rand4 over ACGT with one N takes 1.98-2.08 x the per-call time of the two-plane
 * text of the same symbols (planes3_scan 2.15-2.37 x planes_scan's kernel time), smartgpu_psearch_mis64 at k = 1 / 3 / 7
 * 1.88-2.06 / 1.80-1.97 / 1.68-1.87 x per call, outside the run-to-run spread in every cell.  Against the byte text's best of
 * SO / BNDM / HOR for the same pattern on the same text: 1.27-1.42 x the symbols per second on ACGNT, 1.29-1.33 x on rand8 —
 * the byte text is faster in no measured cell, but a three-plane text is NOT at the two-plane text's 2.7-3.9 x.  Packing:
 * 0.66-0.68 ms per GiB of text.
 * NOT measured: the find forms' speed, set patterns proper (the cells are byte patterns: singleton sets), six and seven
 * values, texts beyond 1 Gi symbols, texts with long partial matches, other occupancies (every planes3 kernel is bounded for
 * 128 VGPRs and launched at 5-7 workgroups per CU). */
#define SMARTGPU_PTEXT_MAXVALUES 8
/* smartgpu_ptext_layout for 1..8 values: 1 / 2 / 3 planes for at most 2 / 4 / 8.  SMARTGPU_ERR_ARG for nvalues < 1 or > 8. */
int smartgpu_ptext_layout8(uint64_t n, int nvalues, int *planes, uint64_t *plane_bytes);   /* 1..8 values: 1 / 2 / 3 planes */
smartgpu_ptext *smartgpu_ptext_pack8(const smartgpu_text *t);
smartgpu_ptext *smartgpu_ptext_upload8(const void *host, uint64_t n, int device);
/* returns k <= 8, the number of distinct values; values[code] = the byte value of each code, ascending (entries from k on: 0) */
int smartgpu_ptext_symbols8(const smartgpu_ptext *t, uint8_t values[8]);
/* smartgpu_iupac_sets, rule for rule, for 1 to 8 values.  A value of the text that is no base letter — 'N', a separator —
 * stands for NO base, so no letter accepts it, pattern letter N included: AN UNKNOWN BASE OF THE TEXT MATCHES NOTHING (a
 * pattern N accepts A, C, G and T; it does not accept the text's N).  Allow it with a mismatch (smartgpu_psearch_sets_mis64)
 * or by setting its bit in sets[j] yourself. */
int smartgpu_iupac_sets8(const uint8_t values[8], int nvalues, const char *P, uint32_t m, uint8_t *sets);

#ifdef __cplusplus
}
#endif
#endif /* SMARTGPU_H */
