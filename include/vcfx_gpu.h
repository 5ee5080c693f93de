/*
 * vcfx_gpu.h -- C ABI of the MI355X VCF record engine (libvcfx_gpu.so).
 *
 * The drop-in boundary for VCFX's per-line hot path.  The reference has no FFI for this
 * path: its callers reach it through the VCFX_<tool> processes, whose
 * main()s are re-implemented in vcfx_amd/csrc/tools/ on top of this ABI.  Each entry
 * point below names the reference function(s) whose per-record work it replaces.
 *
 * Conventions: plain pointers and sizes; every function returns VCFXG_OK (0) or a
 * negative vcfxg_status and never throws; buffers are caller-owned unless stated; one
 * vcfxg_ctx per device, used by one host thread; all work is ordered on the context's
 * HIP stream (vcfxg_stream()).  There is no CPU fallback: without a usable gfx950 device
 * vcfxg_open() fails with VCFXG_E_NODEV.
 */
#ifndef VCFX_GPU_H
#define VCFX_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vcfxg_ctx vcfxg_ctx;

enum vcfxg_status {
    VCFXG_OK = 0,
    VCFXG_E_NODEV = -1,   /* no HIP device / not gfx950 */
    VCFXG_E_HIP = -2,     /* HIP runtime error (vcfxg_last_error has the text) */
    VCFXG_E_ARG = -3,     /* bad argument */
    VCFXG_E_NOMEM = -4,   /* device or host allocation failed */
    VCFXG_E_STATE = -5,   /* call out of order (e.g. no input loaded / not indexed; a result fetch whose
                             call has not run on the current index; a status fetch after another call
                             has written the context's per-line statuses) */
    VCFXG_E_CAP = -6,     /* caller buffer too small */
    VCFXG_E_DATA = -7     /* the input data is invalid (a BGZF member that does not inflate as zlib would) */
};

/* input semantics of the reference tools: file = the mmap path, stdin = the getline path */
enum vcfxg_mode { VCFXG_MODE_FILE = 0, VCFXG_MODE_STDIN = 1 };

/* per-line status codes written by the record kernels (one byte per line of the indexed
 * region) */
enum vcfxg_line_status {
    VCFXG_LINE_SKIP = 0,     /* empty, '#' header, or a data line the tool skips silently */
    VCFXG_LINE_ROW = 1,      /* data line that produces output (AF row / kept record) */
    VCFXG_LINE_DROP = 2,     /* data line evaluated and not kept (filters) */
    VCFXG_LINE_WARN = 3,     /* data line the tool reports on stderr ("fewer than 9 fields") */
    VCFXG_LINE_HEADER = 4,   /* '#' line (pass-through tools print it) */
    VCFXG_LINE_RECHECK = 5   /* vcfxg_record_filter_ex: the line needs strtod's prefix value (host) */
};

typedef struct {
    uint64_t n_lines;      /* lines in the indexed region */
    uint64_t rows;         /* output rows (AF) / kept records (filters) */
    uint64_t data_lines;   /* data lines seen (AF "Processed V variants from L data lines") */
    uint64_t warn_lines;   /* lines flagged VCFXG_LINE_WARN */
    uint64_t text_bytes;   /* bytes of device-formatted output text (AF) */
    uint64_t general_records; /* records that took the general (non fixed-stride) GT path */
} vcfxg_summary;

const char *vcfxg_version(void);
int vcfxg_device_count(int *n);
int vcfxg_open(int device, vcfxg_ctx **out);
void vcfxg_close(vcfxg_ctx *ctx);
/* the device bytes that the buffers of every open context of this process hold (their capacities):
 * exact, and back at its earlier value once a context is closed */
uint64_t vcfxg_device_bytes_live(void);
const char *vcfxg_last_error(const vcfxg_ctx *ctx);
/* the hipStream_t every call of this context is ordered on */
void *vcfxg_stream(vcfxg_ctx *ctx);
/* record HIP events around each kernel launch (see vcfxg_kernel_ms) */
int vcfxg_set_profiling(vcfxg_ctx *ctx, int enable);
/* time only the named kernel (nullptr or "": every kernel); the launches' events are read
   when the figures are asked for, so a profiled loop makes no event queries between calls */
int vcfxg_set_profiling_only(vcfxg_ctx *ctx, const char *kernel);
/* elapsed ms of the last launch of the named kernel ("af_records", "line_index", ...) */
int vcfxg_kernel_ms(vcfxg_ctx *ctx, const char *kernel, float *ms);
/* accumulated event time and launch count of the named kernel since the last reset */
int vcfxg_kernel_stats(vcfxg_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);
int vcfxg_reset_kernel_stats(vcfxg_ctx *ctx);

/* ---- input ---------------------------------------------------------------------------
 * The whole input (file or stdin bytes) is made device-resident once; record kernels read
 * it straight from HBM.  Replaces MappedFile::open (VCFX_allele_freq_calc.cpp:47-70) and
 * the std::getline loops' buffering. */
int vcfxg_load_host(vcfxg_ctx *ctx, const char *host, size_t n);
/* Streaming form of the same (SURVEY 8(b) vcfxg_ingest; the pipe paths of processStdin,
 * VCFX_allele_freq_calc.cpp:477-557, VCFX_record_filter.cpp:498-549, VCFX_genotype_query.cpp:
 * 527-617): vcfxg_ingest_begin starts a new input (size_hint = expected bytes, may be 0);
 * each vcfxg_ingest appends n bytes with an asynchronous H2D copy, so the caller's next read
 * overlaps the transfer; the device buffer grows as needed.  The call with is_final_chunk
 * set completes the input, which is then loaded exactly as by vcfxg_load_host.  Every
 * chunk's host bytes must stay valid until that final call returns.
 * vcfxg_load_host(h, n) == vcfxg_ingest_begin(n) + vcfxg_ingest(h, n, 1). */
int vcfxg_ingest_begin(vcfxg_ctx *ctx, size_t size_hint);
int vcfxg_ingest(vcfxg_ctx *ctx, const char *host, size_t n, int is_final_chunk);
/* wait until the copies of the ingested bytes [0, upto) have completed (their host buffers
 * may then be reused: a pinned staging ring) */
int vcfxg_ingest_wait(vcfxg_ctx *ctx, size_t upto);
/* BGZF (.vcf.gz) input inflated on the device (the reference reads it through zlib,
 * StreamingGzipReader, src/vcfx_core.cpp:144-354, members inflated in sequence with inflateReset
 * at each, :270-277).  Appends the inflated bytes of n_members consecutive BGZF members to the
 * input being ingested: comp[0, comp_n) holds them (host memory), member i = the gzip member at
 * comp[src_off, src_off + src_len) (BSIZE + 1 bytes; the caller has checked its header: gzip magic,
 * CM 8, FLG exactly FEXTRA, the 'BC' subfield) whose trailer's ISIZE is out_len (<= 65536).  The
 * compressed bytes are copied to the device and each member is inflated by one wave, its CRC-32
 * checked against the trailer.  head[0, head_n): the first inflated bytes as the caller has them on
 * the host (the load-time hints are taken from them; may be NULL).  A member whose deflate stream
 * zlib would refuse, that does not end at its trailer, or whose size or CRC-32 differs, fails the
 * call with VCFXG_E_DATA (*bad_member = the first such member) and the ingest is abandoned: the
 * caller then inflates on the host, where zlib reports the damage as the reference does. */
typedef struct {
    uint64_t src_off;  /* the member's first byte in comp */
    uint32_t src_len;  /* the member's bytes (BSIZE + 1) */
    uint32_t out_len;  /* its ISIZE */
} vcfxg_bgzf_member;
int vcfxg_ingest_bgzf(vcfxg_ctx *ctx, const void *comp, size_t comp_n, const vcfxg_bgzf_member *members,
                      size_t n_members, const char *head, size_t head_n, uint64_t *bad_member);
/* The compressed bytes for vcfxg_ingest_bgzf copied to the device piece by piece while the caller
 * still reads the file (a pinned staging ring): bytes [offset, offset + n) of a comp_total-byte
 * stream, in order (offset 0 first; each piece starts where the last ended), asynchronous;
 * vcfxg_ingest_wait(ctx, offset + n) waits for the copy (the host buffer may then be reused).
 * Between vcfxg_ingest_begin and vcfxg_ingest_bgzf, which then takes comp = NULL and
 * comp_n = comp_total. */
int vcfxg_bgzf_stage(vcfxg_ctx *ctx, const void *host, size_t n, size_t offset, size_t comp_total);
/* While staging: launch the inflate of the stream's next `count` members (in chain order from the
 * first; every byte of them already staged), overlapping the copies still to come.  VCFXG_E_CAP:
 * their output does not fit the input buffer as allocated (vcfxg_ingest_begin's size hint) --
 * nothing launched; vcfxg_ingest_bgzf inflates them after growing it.  vcfxg_ingest_bgzf(comp =
 * NULL) then takes the whole member list, launches the members not launched yet and checks every
 * member's CRC-32. */
int vcfxg_bgzf_inflate(vcfxg_ctx *ctx, const vcfxg_bgzf_member *members, size_t count);
/* Members of the last vcfxg_ingest_bgzf that the lane decoder (one member per lane) handed to the
 * wave decoder (one member per wave): stored and fixed-code blocks, codes zlib allows only as a
 * special case, members under 384 bytes, damaged streams (diagnostic; the output is the same). */
uint64_t vcfxg_bgzf_handed_over(const vcfxg_ctx *ctx);
/* page-locked host memory (H2D at the full PCIe rate, asynchronous), for staging rings */
int vcfxg_host_alloc(vcfxg_ctx *ctx, size_t n, void **out);
void vcfxg_host_free(vcfxg_ctx *ctx, void *p);
/* copy input bytes [offset, offset + n) of the loaded input back to host memory (pass-through
 * tools whose stdin was streamed to the device without a host copy write kept records from
 * these) */
int vcfxg_input_fetch(vcfxg_ctx *ctx, uint64_t offset, size_t n, void *host);
/* device copy of the loaded input (read-only view; valid until the next load) */
const void *vcfxg_input_device_ptr(vcfxg_ctx *ctx);

/* ---- K1: record index ------------------------------------------------------------------
 * Newline scan over [data_start, n): line i spans [start_i, end_i) with end_i the offset
 * of its '\n' (or n).  Replaces findNewlineSIMD (VCFX_allele_freq_calc.cpp:150-187,
 * VCFX_record_filter.cpp:28-60, VCFX_genotype_query.cpp:139-171, VCFX_variant_counter.cpp:
 * 46-89, VCFX_ld_calculator.cpp:91-137) and the line loops around them. */
int vcfxg_index(vcfxg_ctx *ctx, size_t data_start, uint64_t *n_lines);
/* copy line end offsets [first, first+count) to host */
int vcfxg_line_ends(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint64_t *out);

/* ---- K2: allele frequency --------------------------------------------------------------
 * Per data line: FORMAT -> GT index, per-sample GT -> (ALT, total) allele counts, freq =
 * alt/total (fp64, correctly rounded), formatted row "CHROM\tPOS\tID\tREF\tALT\t%.4f\n"
 * with the mode's rounding rule.  Replaces processMmap (VCFX_allele_freq_calc.cpp:342-472)
 * and processStdin (:477-557) per-record work: findGTIndex :298-316, extractGT :321-337,
 * parseGenotypeAndCount :262-293, writeDouble4 :119-143 / setprecision(4) :553-555. */
int vcfxg_allele_freq(vcfxg_ctx *ctx, int mode, vcfxg_summary *out);
/* vcfxg_index(data_start) + vcfxg_allele_freq(mode) in one call, with the same results and
 * context state as the two calls (the context is indexed afterwards).  The default device
 * schedule for inputs whose first records average >= 512 B is the walk (one HBM pass: each
 * wave walks the records of one chunk, predicting a record's end from the previous record
 * and validating it by the sample sweep itself); otherwise the index sweep + head pass +
 * sample sweep.  VCFXG_AF_FUSED in the environment at vcfxg_open selects a schedule for
 * measurement: 3 = the two-sweep schedule with the line count read back, 7 = the walk, 8 = the
 * two-sweep schedule with one host synchronisation (all results identical). */
int vcfxg_allele_freq_region(vcfxg_ctx *ctx, size_t data_start, int mode, vcfxg_summary *out);
/* ---- K2: genotype query ----------------------------------------------------------------
 * Per line status (vcfxg_line_status): ROW = some sample's GT sub-field matches `query`
 * (flexible: phase- and order-normalised diploid compare; strict: byte equality), DROP,
 * WARN (fewer than 9 fields), HEADER ('#'), SKIP (empty).  The query is pre-parsed here
 * exactly as main() does (parseDiploidAlleles incl. its partial assignment, then sort).
 * strip_cr evaluates each line without a trailing '\r' (the line as VCFX_record_filter
 * emits it, for the fused record_filter | genotype_query pipeline).  Replaces
 * genotypeQueryMmap / genotypeQueryStream per-record work (VCFX_genotype_query.cpp:433-617):
 * skipToField :223-230, findGTIndex :176-194, extractNthField :199-218,
 * genotypeMatchesFast :275-316, checkAnySampleMatches :322-345. */
int vcfxg_genotype_query(vcfxg_ctx *ctx, const char *query, size_t qlen, int strict, int strip_cr,
                         vcfxg_summary *out);

/* ---- K3: record filter -----------------------------------------------------------------
 * One compiled criterion of VCFX_record_filter (FilterCriterion, VCFX_record_filter.h:37-44,
 * as produced by parseSingleCriterion :89-171): target = 0 POS, 1 QUAL, 2 FILTER, 3 INFO
 * key; op = 0 >, 1 >=, 2 <, 3 <=, 4 ==, 5 !=; numeric = the value parsed fully by strtod
 * (value = that double); key = the INFO key (field name); str = the string value. */
typedef struct {
    int target;
    int op;
    int numeric;
    double value;
    const char *key;
    size_t key_len;
    const char *str;
    size_t str_len;
} vcfxg_criterion;

/* Per line status: ROW = data line passes (AND: all criteria, OR: any), DROP, HEADER ('#',
 * printed without its '\r'), SKIP = empty after '\r' strip (printed as "\n").  Numeric
 * comparisons are exact: strtod(field) is never approximated (see vcfxg_num.h).  Replaces
 * evaluateLine / evaluateCriterion (VCFX_record_filter.cpp:333-401), extractField :207-229,
 * extractInfoValue :234-267, parseDouble :273-299 per record. */
int vcfxg_record_filter(vcfxg_ctx *ctx, const vcfxg_criterion *crit, int n, int and_logic, vcfxg_summary *out);
/* The same with the legacy free-function semantics available (VCFX_record_filter.h:99-102,
 * .cpp:668-805, which no tool calls): flags VCFXG_RF_KEEP_CR evaluates each line with its
 * trailing '\r' (processVCF reads with std::getline); criterion target 4 is QUAL as recordPasses
 * treats it in OR mode (an unparsable QUAL compares as whatever strtod made of it: such lines
 * get status VCFXG_LINE_RECHECK for the caller to decide); a numeric FILTER criterion is passed
 * by the caller as the string criterion recordPasses makes of it. */
#define VCFXG_RF_KEEP_CR 1
int vcfxg_record_filter_ex(vcfxg_ctx *ctx, const vcfxg_criterion *crit, int n, int and_logic, int flags,
                           vcfxg_summary *out);

/* Fused `VCFX_record_filter ... | VCFX_genotype_query ...`: the filter as above, then the
 * genotype query on the lines the filter keeps, evaluated as the filter prints them ('\r'
 * stripped).  Status of a filter-kept data line: ROW = query matches, 6 = no match, 7 =
 * "<9 fields" warning; other lines keep the filter's status. */
int vcfxg_filter_query(vcfxg_ctx *ctx, const vcfxg_criterion *crit, int n, int and_logic, const char *query,
                       size_t qlen, int strict, vcfxg_summary *out);

/* vcfxg_index(data_start) followed by vcfxg_record_filter / vcfxg_genotype_query /
 * vcfxg_filter_query, in one call: the same per-line statuses, line ends, summary and context
 * state (the context is indexed afterwards).  For inputs whose first records average >= 512 B
 * the device walks the records without a separate index sweep (one HBM pass: the walk keeps
 * each record's first 8 tab offsets for the filter, the query's fixed-stride sweep validates
 * the record ends it predicts); VCFXG_FQ_WALK=1 / -1 in the environment at vcfxg_open forces /
 * disables that schedule.  Replace the per-record loops of processFileMmap / processStdin
 * (VCFX_record_filter.cpp:406-549) and genotypeQueryMmap / genotypeQueryStream
 * (VCFX_genotype_query.cpp:433-617) including their line splitting. */
int vcfxg_record_filter_region(vcfxg_ctx *ctx, size_t data_start, const vcfxg_criterion *crit, int n, int and_logic,
                               vcfxg_summary *out);
int vcfxg_genotype_query_region(vcfxg_ctx *ctx, size_t data_start, const char *query, size_t qlen, int strict,
                                int strip_cr, vcfxg_summary *out);
int vcfxg_filter_query_region(vcfxg_ctx *ctx, size_t data_start, const vcfxg_criterion *crit, int n, int and_logic,
                              const char *query, size_t qlen, int strict, vcfxg_summary *out);

/* ---- VCFX_nonref_filter (a per-sample GT reducer on the same path) ----
 * Over the indexed region: per line status 1 keep / 2 drop (every sample hom-ref), 4 '#'
 * line, 0 empty; rows = kept lines, data_lines = evaluated lines, general_records = lines
 * off the fixed-stride sweep.  mode VCFXG_MODE_FILE restates filterNonRefMmap +
 * allSamplesHomRefDirect (VCFX_nonref_filter.cpp:458-551, 248-312; '\r' stripped),
 * VCFXG_MODE_STDIN filterNonRef + isDefinitelyHomRef (:553-636, 419-449).  Data lines
 * before '#CHROM' are the caller's (the tool warns and passes them through). */
int vcfxg_nonref_filter(vcfxg_ctx *ctx, int mode, vcfxg_summary *out);
/* The same over the data region from data_start without a separate index (the filter /
 * query walk with the nonref reducer; index + vcfxg_nonref_filter for short records). */
int vcfxg_nonref_filter_region(vcfxg_ctx *ctx, size_t data_start, int mode, vcfxg_summary *out);

/* ---- VCFX_hwe_tester (a per-sample GT reducer on the same path) -------
 * Over the data region from data_start (the caller passes the end of the leading '#' lines,
 * as performHWE_Mmap's header loop :466-472 skips them): per data line the genotype classes
 * of parseGenotypeForHWE (VCFX_hwe_tester.cpp:339-378) over every sample, the row rules of
 * performHWE_Mmap (:475-558, mode VCFXG_MODE_FILE) or performHWE_Stdin (:572-607, mode
 * VCFXG_MODE_STDIN), and the rows "CHROM\tPOS\tID\tREF\tALT\t<p>\n" with the p-value of
 * calculateHWE_chisq (:278-315) as appendDouble's truncated 6 digits (:236-268, file) or
 * setprecision(6) (stdin).  Text via vcfxg_fetch_text (without the column header line);
 * rows = output rows, general_records = lines off the fixed-stride sweep.  For long records the
 * device walks them as for the allele frequencies (one HBM pass).
 * The p-value's exp() is the device's: a row whose 6 digits it cannot settle (the values a few
 * ulps either side print differently; practically never) is listed by vcfxg_hwe_rechecks, and
 * the caller writes the 8 bytes at text_offset from the host libm's value of the same counts. */
typedef struct {
    uint64_t text_offset; /* offset of the row's 8 p-value bytes in the fetched text */
    int32_t hom_ref, het, hom_alt;
    int32_t reserved;
} vcfxg_hwe_recheck;
int vcfxg_hwe_region(vcfxg_ctx *ctx, size_t data_start, int mode, vcfxg_summary *out);
/* rows of the last vcfxg_hwe_region call that need the host's p-value: *n = their number,
 * the first min(*n, cap) copied to out (any order) */
int vcfxg_hwe_rechecks(vcfxg_ctx *ctx, vcfxg_hwe_recheck *out, uint64_t cap, uint64_t *n);

/* ---- VCFX_dosage_calculator (a per-sample GT map on the same path) ---
 * Over the data lines from data_start (the byte after the '#CHROM' line; data lines before
 * it are the caller's error): per line the row "CHROM\tPOS\tID\tREF\tALT\t" + one dosage
 * per sample (number of non-zero alleles of a diploid GT, or "NA"), comma separated, "NA" for
 * the record when FORMAT has no GT, of processFileMmap (VCFX_dosage_calculator.cpp:375-588,
 * mode VCFXG_MODE_FILE: '\r' stripped) or calculateDosage (:209-360, mode VCFXG_MODE_STDIN);
 * findGTIndexRaw :160-178, extractGTFromSample :182-203, parseDosageInline :111-156 per
 * sample.  Text via vcfxg_fetch_text (without the column header); rows = output rows,
 * warn_lines = lines with fewer than 10 fields (the caller prints the warning),
 * general_records = lines off the fixed-stride sweep; per-line statuses via
 * vcfxg_fetch_lines (1 row, 3 warning, 0 skipped). */
int vcfxg_dosage_region(vcfxg_ctx *ctx, size_t data_start, int mode, vcfxg_summary *out);

/* ---- VCFX_missing_detector (a per-sample GT predicate on the same path) -
 * Over the lines from data_start (the caller passes the end of the leading '#' lines): per
 * line status 0 empty (after the file mode's '\r' strip), 4 '#' line, 1 data line kept as it
 * is, VCFXG_LINE_MISSING a data line with a missing genotype -- some sample's first ':' sub-
 * field holds a '.' that starts or ends it or touches '/' or '|' (hasMissingGenotypeInSamples,
 * VCFX_missing_detector.cpp:290-336).  vcfxg_fetch_lines gives the statuses and, as alt /
 * total, a flagged line's INFO field [start, end) relative to the line start (the caller
 * writes "MISSING_GENOTYPES=1" into it).  mode VCFXG_MODE_FILE: processMmapZeroCopy
 * (:450-589, '\r' dropped); VCFXG_MODE_STDIN: detectMissingGenotypes (:860-911).
 * data_lines = data lines, rows = flagged lines, general_records = lines ending in '\n' whose
 * sample columns hold any '.' (0: the file mode's pre-scan, sampleColumnsHaveAnyDots
 * :371-445, passes the input through unchanged). */
#define VCFXG_LINE_MISSING 6
int vcfxg_missing_region(vcfxg_ctx *ctx, size_t data_start, int mode, vcfxg_summary *out);

/* ---- VCFX_allele_counter (a per-sample GT reducer, a row per sample) ----
 * Over the indexed lines [first_line, last_line): per data line (non-empty, not '#'; no '\r'
 * handling, as in the reference) the REF / ALT allele counts of parseGenotypeRaw
 * (VCFX_allele_counter.cpp:267-294: digit runs of the sample's GT, 0 counting as REF) for each
 * output slot's sample, formatted as the reference does:
 *   kind 0: "CHROM\tPOS\tID\tREF\tALT\t<name>\t<ref>\t<alt>\n" per slot,
 *   kind 1: "CHROM\tPOS\tID\tREF\tALT\t<sum ref>\t<sum alt>\t<rows>\n" per record,
 *   kind 2: the two counts as int8 bytes per slot.
 * seq 0 = countAllelesMmapMT / processChunk (:550-642, 786-950): every slot a row, a sample past
 * the record's last tab counts 0 / 0, counts printed as int8_t; seq 1 = countAllelesUnified
 * (:1266-1468) / countAllelesStream (:1122-1260): a forward-only cursor (a slot reads the
 * largest index so far), rows stop at the first sample that starts at or past the line end.
 * Text (without the column header) via vcfxg_fetch_text / vcfxg_fetch_text_range; per-line
 * statuses via vcfxg_fetch_lines (1 data line, 4 '#CHROM' line, 0 other).  rows = output rows,
 * data_lines = data lines, warn_lines = '#CHROM' lines in the range (countAllelesStream
 * re-selects at each: the caller splits the range there), general_records = lines off the
 * fixed-stride sweep. */
typedef struct {
    const uint32_t *sample;   /* per output slot: the sample's index (sampleIndices) */
    uint64_t m;               /* output slots */
    const char *names;        /* the slots' sample names, concatenated */
    const uint64_t *name_off; /* m + 1 offsets into names */
    int seq;                  /* selection semantics (above) */
    int kind;                 /* 0 text, 1 aggregate, 2 binary */
} vcfxg_ac_params;
int vcfxg_allele_counter(vcfxg_ctx *ctx, uint64_t first_line, uint64_t last_line, const vcfxg_ac_params *params,
                         vcfxg_summary *out);

/* ---- VCFX_inbreeding_calculator (a row per SAMPLE, accumulated over every record) -----------
 * Over the lines from data_start (the caller passes the end of the header lines it parsed): per
 * record the genotype codes of parseGenotypeCode (VCFX_inbreeding_calculator.cpp:296-339: the GT
 * prefix up to the first ':', "a/b" or "a|b" with anything after the second digit run ignored;
 * 0/0 = 0, 0/1 = 1, 1/1 = 2, an allele above 1 or a '.' = -1), then per sample, in record order,
 *   sumExp += 2 freq (1 - freq), obsHet += (code == 1), usedCount++
 * with freq = (altSum - code) / (2 (nGood - 1)) (freq_mode 0, excludeSample) or altSum /
 * (2 nGood) (freq_mode 1, global); skip_boundary drops freq <= 0 or >= 1, and
 * count_boundary_as_used still counts such a record in usedCount (:596-626).  sumExp is the
 * reference's fp64 sum bit for bit: the same operands added in the same order.
 * mode VCFXG_MODE_FILE = calculateInbreedingMmap (:536-629): '\r' stripped, empty / '#' lines,
 * an empty ALT, an ALT with a comma and lines without a tenth field skipped; only the sample
 * columns that start before the line end are parsed, and a sample past them keeps the code of
 * the last parsed record (the reused genotypeCodes buffer, zeros at first).  VCFXG_MODE_STDIN =
 * calculateInbreedingStdin (:689-777): lines of fewer than 10 fields and an ALT with a comma
 * skipped, a sample without a column is -1.  A record is used when at least two codes are >= 0.
 * The text (vcfxg_fetch_text) holds one row per sample, "<name>\tNA\n", "<name>\t1.000000\n" or
 * "<name>\t<F>\n" with F = 1 - obsHet / sumExp in appendDouble's digits (:230-266, :645-663),
 * without the column header.  rows = used records, data_lines = parsed records,
 * general_records = parsed records off the fixed-stride sweep, n_lines = lines from data_start.
 * The records are processed in blocks of VCFXG_IB_BLOCK lines (read by vcfxg_open; default
 * 65536; on the walk schedule rounded to whole walkers, at least one) with the per-sample state
 * kept on the device; the schedule follows VCFXG_AF_FUSED (7 the walk, 3 / 8 the line index) and
 * VCFXG_WALK_CHUNK as the other region calls do. */
typedef struct {
    uint32_t n_samples;          /* the header's sample count (> 0) */
    const char *names;           /* the sample names, concatenated */
    const uint64_t *name_off;    /* n_samples + 1 offsets into names */
    int freq_mode;               /* 0 excludeSample, 1 global */
    int skip_boundary;           /* --skip-boundary */
    int count_boundary_as_used;  /* --count-boundary-as-used */
} vcfxg_ib_params;
int vcfxg_inbreeding_region(vcfxg_ctx *ctx, size_t data_start, int mode, const vcfxg_ib_params *params,
                            vcfxg_summary *out);
/* the last vcfxg_inbreeding_region call's per-sample accumulators (n_samples each; any may be
 * NULL): sumExp, obsHet and usedCount of :527-529 */
int vcfxg_inbreeding_samples(vcfxg_ctx *ctx, double *sum_exp, uint64_t *obs_het, uint64_t *used);

/* ---- VCFX_sample_extractor (a text rewrite: the kept columns of every line) -------------------
 * Over the indexed lines [first_line, last_line), at most VCFXG_SX_BLOCK of them a call (read by
 * vcfxg_open; default 65536): the call takes the lines [first_line, first_line + n_lines) and the
 * caller goes on from there, so the device text stays bounded (a line is at most its own bytes +
 * 2 m + 1).  Number a line's fields from 0 and give a tab the number of the field it precedes: a
 * written line is its bytes numbered 0..8 and those numbered cols[i], "\t." for every cols[i] the
 * line has no field for, and '\n' (extractSamplesMmap, VCFX_sample_extractor.cpp:287-332;
 * extractSamples :512-533).  Per line status (vcfxg_fetch_lines) and text (vcfxg_fetch_text /
 * vcfxg_fetch_text_range, in line order):
 *   VCFXG_SX_EMPTY      an empty line: "\n" (:216-220, :461-464)
 *   VCFXG_SX_HEADER     a '#' line, copied (:271-275, :497-500)
 *   VCFXG_SX_ROW        a data line, written as above
 *   VCFXG_SX_SHORT      fewer than 8 fields: nothing; "line has <8 columns" (:311-315, :513-516)
 *   VCFXG_SX_NO_SAMPLES stdin mode, exactly 8 fields: nothing; "data line with no sample columns"
 *                       (:517-520; file mode writes the 8 fields and "\t." per kept column)
 *   VCFXG_SX_PRE        a data line and seen_chrom == 0: nothing; "data line encountered before
 *                       #CHROM" (:281-285, :508-511)
 *   VCFXG_SX_CHROM      stdin mode, a line that starts with "#CHROM": nothing.  The reference
 *                       selects again there (:466-496): the caller splits its range at such a line,
 *                       writes the line itself and goes on with the new columns.  (File mode
 *                       rewrites only the first one, :224, which the caller handles before the
 *                       range; a later one is a VCFXG_SX_HEADER line.)
 * mode VCFXG_MODE_FILE strips one trailing '\r' from every line first (:212-214), VCFXG_MODE_STDIN
 * none, so there the '\r' belongs to the last field and stays only when that column is kept.
 * cols: the kept columns' field numbers (>= 9), ascending; m = 0 is legal (fields 0..8 only).
 * rows = lines written (VCFXG_SX_ROW), data_lines = non-empty lines that are not '#' lines,
 * warn_lines = lines the caller has to act on (SHORT, NO_SAMPLES, PRE and CHROM), text_bytes,
 * n_lines = the lines taken by this call. */
#define VCFXG_SX_EMPTY 0
#define VCFXG_SX_ROW 1
#define VCFXG_SX_SHORT 3
#define VCFXG_SX_HEADER 4
#define VCFXG_SX_NO_SAMPLES 5
#define VCFXG_SX_PRE 6
#define VCFXG_SX_CHROM 7
typedef struct {
    const uint32_t *cols; /* kept columns: field numbers >= 9, strictly ascending */
    uint64_t m;           /* their count (0: none) */
    int mode;             /* VCFXG_MODE_FILE / VCFXG_MODE_STDIN */
    int seen_chrom;       /* a '#CHROM' line precedes first_line */
} vcfxg_sx_params;
int vcfxg_sample_extract(vcfxg_ctx *ctx, uint64_t first_line, uint64_t last_line, const vcfxg_sx_params *params,
                         vcfxg_summary *out);

/* ---- VCFX_multiallelic_splitter (a value-dependent rewrite: one line per ALT allele) -----------
 * Over the indexed lines [first_line, last_line), at most VCFXG_MS_BLOCK of them a call (read by
 * vcfxg_open; default 65536) and no more than fit VCFXG_MS_BYTES of text (default 512 MiB; a
 * line counts as nAlts x (its bytes + 1), and one line is always taken): the call takes the lines
 * [first_line, first_line + n_lines) and the caller goes on from there.  A data line of >= 9
 * fields whose ALT holds a comma is split: row a of its nAlts rows keeps fields 0-3, ALT piece a,
 * fields 5-6 and FORMAT, and recodes INFO and every sample for that allele (recodeInfoField /
 * recodeSample, VCFX_multiallelic_splitter.cpp:247-420).  Fields are counted as
 * VCFXG_MODE_FILE's splitTabsView (:22-38: a line that ends in a tab has no trailing empty
 * field) or VCFXG_MODE_STDIN's vcfx::split_tabs (it has); '\r' is never stripped.
 * Per line status and nAlts (vcfxg_fetch_lines: status, alt):
 *   VCFXG_MS_EMPTY   an empty line (stdin mode writes "\n", file mode nothing: the caller's)
 *   VCFXG_MS_HEADER  a '#' line, copied by the caller
 *   VCFXG_MS_COPY    a data line that is not split, copied by the caller; alt = 0
 *   VCFXG_MS_SPLIT   a split line; alt = nAlts
 * The device text (vcfxg_fetch_text_range) holds only the rows of the SPLIT lines, in line order
 * and allele order, each with its '\n'; vcfxg_ms_line_ranges gives every line's place in it.
 * table: the ##INFO / ##FORMAT declarations in header order, n_entries of them; the last entry
 * of an ID wins across both sections (parseHeaderLine :226-245), and only that one counts.  The
 * first VCFXG_MS_KEYS_LDS FORMAT keys of a line have their classes in LDS, and a table of up to
 * VCFXG_MS_TABLE_LDS bytes (12 per ID + the ID's bytes rounded up to 4) sits there too; lines
 * past either cap take global look-ups and are counted in general_records.
 * rows = output rows written, data_lines = COPY + SPLIT lines, n_lines = the lines taken,
 * text_bytes.  Outside the domain: a GT allele index of more than 9 digits, an ALT of 46,340 or
 * more alleles (the reference's int arithmetic overflows), a line of 2 GiB or more. */
#define VCFXG_MS_EMPTY 0
#define VCFXG_MS_COPY 1
#define VCFXG_MS_SPLIT 2
#define VCFXG_MS_HEADER 4
#define VCFXG_MS_INFO 0
#define VCFXG_MS_FORMAT 1
#define VCFXG_MS_NUM_OTHER 0
#define VCFXG_MS_NUM_A 1
#define VCFXG_MS_NUM_R 2
#define VCFXG_MS_NUM_G 3
#define VCFXG_MS_KEYS_LDS 32
#define VCFXG_MS_TABLE_LDS 16384
typedef struct {
    const char *id;   /* the ID's bytes */
    uint32_t id_len;
    uint8_t section;  /* VCFXG_MS_INFO / VCFXG_MS_FORMAT */
    uint8_t number;   /* VCFXG_MS_NUM_* */
} vcfxg_ms_entry;
typedef struct {
    const vcfxg_ms_entry *table;
    uint64_t n_entries;
    int mode;         /* VCFXG_MODE_FILE / VCFXG_MODE_STDIN */
} vcfxg_ms_params;
int vcfxg_multiallelic_split(vcfxg_ctx *ctx, uint64_t first_line, uint64_t last_line, const vcfxg_ms_params *params,
                             vcfxg_summary *out);
/* off[i] = the text offset of the rows of line first + i of the last vcfxg_multiallelic_split's
 * block, count + 1 entries (a line that is not split has an empty range) */
int vcfxg_ms_line_ranges(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint64_t *off);

/* ---- VCFX_fasta_converter (the first transpose: a row per SAMPLE, a byte per record) ------------
 * Over the indexed lines [first_line, last_line), at most VCFXG_FA_BLOCK of them a call (read by
 * vcfxg_open; default 65536): the call takes the lines [first_line, first_line + n_lines) and the
 * caller goes on from there.  Per line status (vcfxg_fasta_status):
 *   VCFXG_FA_EMPTY    an empty line on stdin (skipped, VCFX_fasta_converter.cpp:444)
 *   VCFXG_FA_HEADER   a '#' line, skipped wherever it stands (:311-328, :359, :446-462)
 *   VCFXG_FA_CHROM    a line that starts with "#CHROM": the caller reads its names (fields 10 on)
 *   VCFXG_FA_SKIPPED  stdin: a data line of fewer than 9 + n_samples fields (:480; a line that ends
 *                     in a tab has no empty last field)
 *   VCFXG_FA_COLUMN   a variant: VCFXG_MODE_FILE every line that does not start with '#', the empty
 *                     ones too (:330-333); VCFXG_MODE_STDIN every other non-empty line
 * A column's base for sample k (the k-th tab-separated field from the tenth on; file mode strips one
 * '\r' from the line first, stdin mode none) is parseGenotype's (:198-224): N without a FORMAT key
 * that is exactly GT, for an empty or '.'-led GT sub-field, without '/' or '|' after the first
 * number, or when either allele's base is N; the base of allele 0 is REF when it is one byte
 * (upper-cased as the mode does, :365 / :486), of allele k >= 1 the k-th ALT piece when it is one
 * letter (parseAlleleBase :180-196); equal bases give that base, A/C/G/T pairs their IUPAC letter,
 * anything else N.  A sample the line has no field for is the byte 0 (file mode's zeroed matrix).
 * vcfxg_fasta_scan: the statuses and each line's column number within the block (n_samples: the
 * stdin field rule); rows = columns, warn_lines = "#CHROM" lines, n_lines = the lines taken.
 * vcfxg_fasta_begin sizes the text; vcfxg_fasta scans a block the same way, writes its columns'
 * bases into a record-major matrix and transposes it into the text: column first_col + c of the
 * block, sample s, is text byte row_off[s] + c' + c' / 60 with c' = first_col + c - skip[s] (columns
 * below skip[s] are not written; skip NULL = all zero), each followed by '\n' when c' % 60 = 59 or
 * c' + skip[s] + 1 = total_cols.  The text (vcfxg_fetch_text_range) holds the sequence lines only;
 * the caller writes ">name\n" before each row.  general_records = the columns that left the
 * fixed-stride path (GT first in FORMAT and every sample "a s b" with one separator and a, b in
 * [0-9.]), rows = the block's columns, text_bytes = the size given to vcfxg_fasta_begin.
 * Outside the domain: an allele index of more than 9 digits, a line of 2 GiB or more. */
#define VCFXG_FA_EMPTY 0
#define VCFXG_FA_COLUMN 1
#define VCFXG_FA_SKIPPED 3
#define VCFXG_FA_HEADER 4
#define VCFXG_FA_CHROM 7
#define VCFXG_FA_LINE 60
#define VCFXG_FA_TILE_SAMPLES 64
#define VCFXG_FA_TILE_COLUMNS 240
#define VCFXG_FA_TABLE 16
typedef struct {
    int mode;                /* VCFXG_MODE_FILE / VCFXG_MODE_STDIN */
    uint32_t n_samples;      /* the names these lines are parsed against */
    uint64_t first_col;      /* the block's first column among all columns */
    uint64_t total_cols;     /* all columns of the input */
    const uint64_t *row_off; /* n_samples text offsets (host) */
    const uint64_t *skip;    /* n_samples: columns before each sample's "#CHROM" line; NULL = none */
} vcfxg_fa_params;
int vcfxg_fasta_scan(vcfxg_ctx *ctx, uint64_t first_line, uint64_t last_line, int mode, uint32_t n_samples,
                     vcfxg_summary *out);
/* statuses (and, when col is not NULL, column numbers within the block: the columns before each
 * line) of lines [first, first + count) of the last vcfxg_fasta_scan / vcfxg_fasta block */
int vcfxg_fasta_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status, uint64_t *col);
int vcfxg_fasta_begin(vcfxg_ctx *ctx, uint64_t text_bytes);
int vcfxg_fasta(vcfxg_ctx *ctx, uint64_t first_line, uint64_t last_line, const vcfxg_fa_params *params,
                vcfxg_summary *out);

/* ---- VCFX_cross_sample_concordance (a set question per record: its distinct genotypes) --------
 * Over the lines from data_start (the byte after the first '#CHROM' line): per record the keys of
 * parseGenotypeToId (VCFX_cross_sample_concordance.cpp:130-167: the first ':' sub-field, digits,
 * one '/' or '|', digits, an empty run reading as 0, anything after ignored; invalid when it
 * starts with '.', lacks the separator, or an allele is above numAlt of countAltAlleles :170-178
 * or above 127; the key is the sorted pair) over the selected sample columns; N = the valid keys
 * (each counted as often as its column is selected), U = the distinct ones; the row
 * "CHROM\tPOS\tID\tREF\tALT\t<N>\t<U>\tCONCORDANT|DISCORDANT\n", or "...\t0\t0\tNO_GENOTYPES\n"
 * when N = 0.  mode VCFXG_MODE_FILE = calculateConcordanceMmapParallel + processVariantLine
 * (:229-319, :445-581): '\r' stripped, empty and '#' lines dropped, a row for a line of >= 5
 * fields with a non-empty CHROM, selected columns past the line skipped; with threads = T > 0 the
 * rows stand in the reference's order for T workers (clamped to the data lines; worker t takes
 * data lines t, t + T, ... and the workers' rows follow one another), written there directly.
 * VCFXG_MODE_STDIN = calculateConcordance (:649-716): no strip, a row for a line of at least
 * max(8, 9 + n_samples) fields; pass threads = 0 (record order).
 * Text via vcfxg_fetch_text (without the column header); per line via vcfxg_fetch_lines: alt = N,
 * total = U, status 0 no row / VCFXG_CC_CONCORDANT / VCFXG_CC_DISCORDANT / VCFXG_CC_NO_GENOTYPES.
 * rows = output rows, data_lines = the collected data lines (non-empty, not '#'), n_lines,
 * text_bytes.  For long records whose every header column is selected once (mult NULL or all
 * ones) the device counts the fixed-stride records on the record walk (one HBM pass) and parses
 * only the lines it leaves with the per-line kernel; otherwise that kernel takes every line after
 * the line index.  general_records = the data lines the per-line kernel parsed.  The schedule
 * follows VCFXG_AF_FUSED (7 the walk, 3 / 8 the line index) and VCFXG_WALK_CHUNK as the other
 * region calls do; the context is indexed afterwards.
 * Two things are undefined in the reference and not reproduced: a digit run that overflows int,
 * and a file-mode row longer than 4,095 bytes. */
#define VCFXG_CC_CONCORDANT 1
#define VCFXG_CC_DISCORDANT 2
#define VCFXG_CC_NO_GENOTYPES 3
typedef struct {
    uint32_t n_samples;   /* the header's sample count (stdin mode's field rule; the columns selected when mult is NULL) */
    const uint32_t *mult; /* per sample column (field 9 + i) how often it is selected: 0 = not, 2 and
                             more = repeated '#CHROM' lines; NULL = each of the first n_samples once */
    uint64_t n_mult;      /* entries of mult */
    uint64_t threads;     /* T of the file mode's row order; 0 = record order */
} vcfxg_cc_params;
int vcfxg_concordance_region(vcfxg_ctx *ctx, size_t data_start, int mode, const vcfxg_cc_params *params,
                             vcfxg_summary *out);
/* the last vcfxg_concordance_region call's totals: concordant, discordant and no-genotype rows,
 * data lines */
int vcfxg_concordance_totals(const vcfxg_ctx *ctx, uint64_t totals[4]);
/* the start offsets, ascending, of the lines from data_start that begin with "#CHROM" (the file
 * mode reads every one of them before any record): *n = their number; when it exceeds cap the
 * caller repeats the call with room for all.  The context is indexed from data_start afterwards. */
int vcfxg_chrom_lines(vcfxg_ctx *ctx, size_t data_start, uint64_t *starts, uint64_t cap, uint64_t *n);

/* ---- VCFX_duplicate_remover (a question across records: has an earlier line the same key) ------
 * Over the indexed lines (vcfxg_index, from offset 0 for the tool): a data line is kept when no
 * earlier data line has the same (CHROM bytes, POS integer, REF bytes, multiset of ALT tokens);
 * ID and everything after ALT are not compared (removeDuplicates, VCFX_duplicate_remover.cpp:
 * 182-214; processFileMmap :226-382).  Lines end at '\n' only; a '\r' is a byte of its field.
 * Per line status (vcfxg_dedup_status):
 *   VCFXG_DD_EMPTY   an empty line: dropped silently (:191-193, :281-284)
 *   VCFXG_DD_HEADER  a line that starts with '#', wherever it stands: written (:194-197, :287-297)
 *   VCFXG_DD_SHORT   a data line with fewer than four tabs: dropped, "Warning: Skipping invalid
 *                    VCF line." (:200-205, :305-345)
 *   VCFXG_DD_KEPT    a data line whose key no earlier line has: written
 *   VCFXG_DD_DUP     a data line whose key an earlier line has: dropped
 * ALT runs to the fifth tab or the line's end.  VCFXG_MODE_STDIN: POS = std::stoi of the field, 0
 * on any exception (no digits, outside int); ALT split at every comma, empty tokens included
 * (:111-134).  VCFXG_MODE_FILE: POS = (int)strtol from the field's first byte, whose white-space
 * skip runs across tabs and newlines into the following fields or lines, saturating at LONG_MAX /
 * LONG_MIN before the cast; empty ALT tokens dropped (:137-180).  Outside the domain: an input
 * with NUL bytes, and a file-mode POS scan that reaches the input's end (the reference reads past
 * its mapping there; this engine stops at the end).
 * The device hashes each key (ALT as a commutative sum of token hashes: no order, no sorting),
 * sorts (hash, line) stably and compares every line exactly with the first line of its run of
 * equal hashes; lines that differ from it are resolved in line order against the run's kept
 * lines, so the result does not depend on the hash.  hash_bits masks the hash before the sort.
 * A line whose ALT ends within its first VCFXG_DD_WINDOW bytes and whose POS is 1..9 digits is
 * parsed by one lane; every other line by a wave (general_records counts those).
 * rows = kept lines, data_lines = kept + duplicate lines, warn_lines = SHORT lines, n_lines. */
#define VCFXG_DD_EMPTY 0
#define VCFXG_DD_KEPT 1
#define VCFXG_DD_DUP 2
#define VCFXG_DD_SHORT 3
#define VCFXG_DD_HEADER 4
#define VCFXG_DD_WINDOW 64
typedef struct {
    uint32_t hash_bits; /* 0: all 64 bits; 1..63: only the low bits (tests force collisions) */
} vcfxg_dd_params;
int vcfxg_dedup(vcfxg_ctx *ctx, int mode, const vcfxg_dd_params *params, vcfxg_summary *out);
/* the statuses of lines [first, first + count) of the last vcfxg_dedup on this index (read them
 * before another per-line call of this context writes its own); VCFXG_E_STATE without one */
int vcfxg_dedup_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status);
/* the last vcfxg_dedup's lines per status (counts[VCFXG_DD_EMPTY .. VCFXG_DD_HEADER]) and, in
 * counts[5], the lines the wave path parsed */
int vcfxg_dedup_counts(const vcfxg_ctx *ctx, uint64_t counts[6]);

/* ---- VCFX_sorter (a permutation of the records: the lines in (CHROM, POS) order) ---------------
 * Over the indexed lines (vcfxg_index, from offset 0 for the tool): the '#' lines in input order,
 * then the kept data lines in key order (sortFileMmap, VCFX_sorter.cpp:321-459; sortExternal
 * :601-674).  Lines end at '\n' only; a '\r' is a byte of its line.  Per line status
 * (vcfxg_sort_status):
 *   VCFXG_SRT_EMPTY   an empty line: file mode drops it, stdin mode writes "\n" among the '#' lines
 *   VCFXG_SRT_HEADER  a line that starts with '#', wherever it stands: written first, in input order
 *   VCFXG_SRT_PRE     file mode, a data line before the first line that starts with "#CHROM":
 *                     dropped, "Warning: data line before #CHROM => skipping."
 *   VCFXG_SRT_BAD     dropped, "Warning: skipping malformed line."  File mode: no tab, or a POS
 *                     (the digits after the first tab, accumulated in a wrapping 32-bit int) of
 *                     0; a value that wrapped negative is kept and sorts as a negative int, as in
 *                     the compiled reference.  Stdin mode: fewer than two tabs, or a POS field std::stoi
 *                     refuses (white space, one sign, digits; no digits or a value outside int).
 *   VCFXG_SRT_KEPT    a data line of the output
 * Order.  natural = 0: CHROM as unsigned bytes (a prefix before its extensions), then POS; an
 * empty CHROM first in file mode and last in stdin mode (chromToId's 999999 there).  natural = 1:
 * (chromToId, POS) as two ints (:43-146; names that share an id are one chromosome).  EQUAL KEYS
 * KEEP THEIR INPUT ORDER: the reference's std::sort leaves them in whatever order its C++ library
 * does (stable up to 16 kept lines with libstdc++), so the outputs are byte-identical when no two
 * kept lines share a key and otherwise differ only inside runs of equal keys.
 * The device sorts exactly for any CHROM length and any byte values (an LSD radix sort over POS,
 * the length and CHROM's 8-byte words), then gathers the lines into the text, at most
 * VCFXG_SRT_BLOCK bytes a call (read by vcfxg_open; default 256 MiB), one line at least:
 * vcfxg_sort_text takes output lines [first_out_line, first_out_line + *lines_taken), each with a
 * '\n' (a final input line without one gets it), as text bytes [0, *bytes) (vcfxg_fetch_text_range),
 * and the caller goes on from there.  A line whose key fields end within its first
 * VCFXG_SRT_WINDOW bytes is parsed by one lane, every other line by a wave (general_records).
 * rows = written lines, data_lines = kept data lines, warn_lines = PRE + BAD lines, n_lines.
 * Outside the domain: a digit run in CHROM (natural order) or a stdin-mode POS whose value the
 * reference's own arithmetic leaves undefined. */
#define VCFXG_SRT_EMPTY 0
#define VCFXG_SRT_KEPT 1
#define VCFXG_SRT_PRE 2
#define VCFXG_SRT_BAD 3
#define VCFXG_SRT_HEADER 4
#define VCFXG_SRT_WINDOW 64
typedef struct {
    int natural; /* 0: lexicographic CHROM order; 1: -n / --natural-chr */
} vcfxg_srt_params;
int vcfxg_sort(vcfxg_ctx *ctx, int mode, const vcfxg_srt_params *params, vcfxg_summary *out);
/* the statuses of lines [first, first + count) of the last vcfxg_sort on this index (read them
 * before another per-line call of this context writes its own); VCFXG_E_STATE without one */
int vcfxg_sort_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status);
/* the last vcfxg_sort's lines per status (counts[VCFXG_SRT_EMPTY .. VCFXG_SRT_HEADER]) and, in
 * counts[5], the lines the wave path parsed */
int vcfxg_sort_counts(const vcfxg_ctx *ctx, uint64_t counts[6]);
/* the input line numbers of output lines [first, first + count) of the last vcfxg_sort */
int vcfxg_sort_order(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint32_t *lines);
int vcfxg_sort_text(vcfxg_ctx *ctx, uint64_t first_out_line, uint64_t *lines_taken, uint64_t *bytes);

/* ---- VCFX_diff_tool (the first join of two inputs: which variant keys has only one file) --------
 * Both files are ONE input: file 1's bytes, one '\n' when file 1 is not empty and lacks a final one,
 * then file 2's bytes (vcfxg_ingest takes them as chunks), indexed from offset 0.  second_start is
 * the byte where file 2 begins; the call finds the cut line itself (the first line that starts at or
 * after it).  Lines end at '\n' only; NUL bytes and bytes >= 0x80 are ordinary bytes.  Per line
 * status (vcfxg_diff_status; parseVariantLine, VCFX_diff_tool.cpp:214-264):
 *   VCFXG_DF_EMPTY    an empty line
 *   VCFXG_DF_HEADER   a line that starts with '#'
 *   VCFXG_DF_SKIPPED  a line that, after one trailing '\r' is dropped, has fewer than four tabs, or
 *                     whose POS field holds a byte outside 0-9 (an empty POS passes): no warning
 *   VCFXG_DF_UNIQUE   a data line whose key is printed
 *   VCFXG_DF_COMMON   a data line whose key the other file cancels
 *   VCFXG_DF_REPEAT   default mode: a data line whose key an earlier line of the same file carries
 * The key is the text CHROM:POS:REF:ALT' (generateVariantKey :168-200): POS as its bytes, ALT' =
 * ALT (to the fifth tab or the line's end) split at every comma, empty tokens kept, the tokens in
 * unsigned byte order (a prefix before its extensions), joined with ','.  Keys are whole strings:
 * different fields that print the same text are the same key.
 * assume_sorted = 0 (diffInMemoryMmap :333-404): the two files' SETS of keys; a line is UNIQUE when
 * it is the first of its file with its key and no line of the other file has that key.  EACH SIDE
 * IS IN INPUT ORDER OF THE KEY'S FIRST LINE; the reference prints each side in the iteration order
 * of its C++ library's unordered_set, so the two outputs hold the same lines in another order.  The
 * device hashes the key text, sorts (hash, line) stably and compares every line exactly with the
 * first line of its run; lines that differ are resolved in line order, so the result does not
 * depend on the hash.  hash_bits masks the hash before the sort.
 * assume_sorted = 1 (diffStreamingMmap :409-506): the two-pointer walk over both files' data lines
 * under compareKeys (:312-328): CHROM as unsigned bytes, or with natural = 1 compareChromNatural
 * (:269-307: a prefix of exactly chr / Chr / CHR dropped, names with a decimal digit prefix first and
 * among themselves by its value, then the rest as bytes); POS as an integer; REF bytes; the raw ALT
 * bytes.  Less: file 1's key is reported; greater: file 2's; equal: neither; what is left is
 * reported; each side in file order, repeats kept.  When both files are non-decreasing the walk is
 * a multiset difference, decided per line by binary searches (VCFXG_DF_PATH_BOUNDS); otherwise the
 * device runs the loop itself, one wave, at most VCFXG_DF_WALK_STEPS steps a launch (read by
 * vcfxg_open; default 2^20) with its pointers in device memory (VCFXG_DF_PATH_WALK).  Outside the
 * domain: a POS or a natural-order digit prefix of more than 18 digits (the reference's long
 * arithmetic overflows).  natural is read only with assume_sorted.
 * A line whose fifth tab lies within its first VCFXG_DF_WINDOW bytes (or that is no longer than
 * that) is parsed by one lane; every other line by a wave (general_records counts those).
 * rows = unique lines of both sides, data_lines, warn_lines = skipped lines, n_lines.
 * vcfxg_diff_counts: unique lines of file 1 and of file 2, data lines of file 1 and of file 2,
 * skipped lines, the lines the wave path parsed, the path taken (VCFXG_DF_PATH_*), the cut line.
 * vcfxg_diff_text: keys [first_out, first_out + *taken) of one side's output (side 0: file 1), each
 * with its '\n', as text bytes [0, *bytes) (vcfxg_fetch_text_range): at most VCFXG_DF_BLOCK bytes a
 * call (read by vcfxg_open; default 256 MiB), one key at least; the caller goes on from
 * first_out + *taken. */
#define VCFXG_DF_EMPTY 0
#define VCFXG_DF_COMMON 1
#define VCFXG_DF_UNIQUE 2
#define VCFXG_DF_SKIPPED 3
#define VCFXG_DF_HEADER 4
#define VCFXG_DF_REPEAT 5
#define VCFXG_DF_WINDOW 64
#define VCFXG_DF_PATH_HASH 0
#define VCFXG_DF_PATH_BOUNDS 1
#define VCFXG_DF_PATH_WALK 2
typedef struct {
    uint64_t second_start; /* the byte where file 2 begins */
    int assume_sorted;     /* -s / --assume-sorted */
    int natural;           /* -n / --natural-chr (with assume_sorted) */
    uint32_t hash_bits;    /* 0: all 64 bits; 1..63: only the low bits (tests force collisions) */
} vcfxg_df_params;
int vcfxg_diff(vcfxg_ctx *ctx, const vcfxg_df_params *params, vcfxg_summary *out);
/* the statuses of lines [first, first + count) of the last vcfxg_diff on this index (read them
 * before another per-line call of this context writes its own); VCFXG_E_STATE without one */
int vcfxg_diff_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status);
int vcfxg_diff_counts(const vcfxg_ctx *ctx, uint64_t counts[8]);
int vcfxg_diff_text(vcfxg_ctx *ctx, int side, uint64_t first_out, uint64_t *taken, uint64_t *bytes);

/* ---- VCFX_merger (the first join of K inputs: their lines in key order) -------------------------
 * The files are ONE input: every opened file in list order, each followed by one '\n' when it is
 * not empty and lacks a final one (vcfxg_ingest takes them as chunks), indexed from offset 0.
 * file_start holds n_files + 1 non-decreasing byte offsets: where each file begins, then the
 * text's size; the call finds each file's first line itself.  Lines end at '\n' only; '\r', NUL
 * and bytes >= 0x80 are ordinary bytes.  Per line status (vcfxg_merge_status):
 *   VCFXG_MG_EMPTY    an empty line: dropped
 *   VCFXG_MG_KEPT     a data line of the output
 *   VCFXG_MG_BAD      a line that does not start with '#' and has fewer than two tabs, or whose POS
 *                     (the bytes between the first two tabs) std::stol refuses: white space, one
 *                     sign, at least one decimal digit, the rest ignored; no digit or a value
 *                     outside a 64-bit long fails (parseChromPos, VCFX_merger.cpp:77-92).  Dropped;
 *                     the default mode warns per line, -s is silent.
 *   VCFXG_MG_HEADER   a '#' line of the output.  assume_sorted = 0 (mergeVCFInMemory :176-254): ALL
 *                     '#' lines, wherever they stand, of the first file that has any.
 *                     assume_sorted = 1 (mergeVCFStreaming :257-345): the '#' lines before the first
 *                     line that is neither empty nor '#', of the first file that has such lines.
 *   VCFXG_MG_DROPPED  every other '#' line
 * The output is the header lines in input order, then the kept lines of all files.
 * Order.  natural = 0: CHROM as unsigned bytes (a prefix before its extensions), then POS as a
 * signed 64-bit integer.  natural = 1 (parseChromNat :43-74): the first three bytes when they are
 * "chr" in any letter case, AS WRITTEN, are the prefix (else it is empty); the decimal digits after
 * it are num, the rest the suffix; the order is prefix bytes, names with digits before names
 * without, num, suffix bytes, POS.  "1" and "01" are equal keys; "chr1" and "Chr1" are not.
 * EQUAL KEYS COME OUT IN (FILE LIST ORDER, LINE ORDER): the reference leaves them to std::sort and
 * to its heap, so the outputs are byte-identical when no two kept lines share a key and otherwise
 * differ only inside runs of equal keys.
 * assume_sorted = 0, and assume_sorted = 1 when every file is non-decreasing: one stable LSD radix
 * sort over POS, the key string's length and its 8-byte words (natural: then num and the prefix),
 * exact for any length and any byte values (VCFXG_MG_PATH_SORT).  assume_sorted = 1 with a file
 * out of order: the reference's heap process itself (pop the least head, the earliest file among
 * equals; push that file's next kept line), one wave, at most VCFXG_MG_WALK_STEPS steps a launch
 * (read by vcfxg_open; default 2^20) with the cursors in device memory (VCFXG_MG_PATH_WALK).
 * Outside the domain: natural = 1 with a digit run of more than 18 digits (the reference then
 * compares uninitialised values).
 * A line whose second tab lies within its first VCFXG_MG_WINDOW bytes (or that is no longer than
 * that) is parsed by one lane; every other line by a wave (general_records counts those).
 * rows = written lines, data_lines = kept lines, warn_lines = BAD lines, n_lines.
 * vcfxg_merge_counts: the lines per status (counts[VCFXG_MG_EMPTY .. VCFXG_MG_DROPPED]), the lines
 * the wave path parsed, the path taken (VCFXG_MG_PATH_*), the header's file (n_files: none).
 * vcfxg_merge_files: each file's first line (n_files + 1 entries, the last one n_lines) and its BAD
 * lines (n_files entries).  vcfxg_merge_order: the input line numbers of output lines
 * [first, first + count).  vcfxg_merge_text: output lines [first_out_line, first_out_line +
 * *lines_taken), each with its '\n', as text bytes [0, *bytes) (vcfxg_fetch_text_range): at most
 * VCFXG_SRT_BLOCK bytes a call (the sorter's bound and gather), one line at least; the caller goes
 * on from there.  Every fetcher returns VCFXG_E_STATE without a vcfxg_merge on this index. */
#define VCFXG_MG_EMPTY 0
#define VCFXG_MG_KEPT 1
#define VCFXG_MG_BAD 2
#define VCFXG_MG_HEADER 3
#define VCFXG_MG_DROPPED 4
#define VCFXG_MG_WINDOW 64
#define VCFXG_MG_PATH_SORT 0
#define VCFXG_MG_PATH_WALK 1
typedef struct {
    const uint64_t *file_start; /* n_files + 1 offsets: where each file begins; the text's size */
    uint32_t n_files;           /* K >= 1 */
    int assume_sorted;          /* -s / --assume-sorted */
    int natural;                /* -n / --natural-chr */
} vcfxg_mg_params;
int vcfxg_merge(vcfxg_ctx *ctx, const vcfxg_mg_params *params, vcfxg_summary *out);
int vcfxg_merge_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status);
int vcfxg_merge_counts(const vcfxg_ctx *ctx, uint64_t counts[8]);
int vcfxg_merge_files(vcfxg_ctx *ctx, uint64_t *first_line, uint64_t *bad);
int vcfxg_merge_order(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint32_t *lines);
int vcfxg_merge_text(vcfxg_ctx *ctx, uint64_t first_out_line, uint64_t *lines_taken, uint64_t *bytes);

/* ---- VCFX_region_subsampler (the first join against a side table: is the record inside a BED) ---
 * The table (vcfxg_regions_load): n_chrom distinct names (their bytes in `names`, name i =
 * [name_off[i], name_off[i + 1])) and n intervals (chrom_id, 1-based start1 >= 1, end >= start1),
 * what loadRegions keeps of a BED (VCFX_region_subsampler.cpp:344-381; the host parses the text).
 * The device sorts the intervals by (name id, start), scans the furthest end along each name (the
 * "reach") and keeps per name its range; the merged intervals the reference builds
 * (sortAndMergeIntervals :383-404: joined when start <= last end + 1) are exported in (name id,
 * start) order by vcfxg_regions_merged (*n = their number; more than cap: nothing is copied and the
 * caller repeats the call with room for all).  The names go into an open-addressing dictionary over
 * their hash; hash_bits masks the hash; every hit is confirmed byte by byte, so no answer depends
 * on the hash.  A table of zero intervals is legal; n < 2^31.  The table stays resident across
 * loads and indexes of the input until the next vcfxg_regions_load.
 * vcfxg_region_filter over the indexed lines (vcfxg_index, from offset 0 for the tool).  Lines end at
 * '\n' only; a '\r' is a byte of its line.  Per line status (vcfxg_region_status), the checks in
 * this order:
 *   VCFXG_RS_EMPTY   an empty line: "\n" written (:451-455, :528-531)
 *   VCFXG_RS_HEADER  a line that starts with '#', wherever it stands: written (:458-466, :532-538)
 *   VCFXG_RS_EARLY   a data line before the first line that starts with "#CHROM": dropped, "Warning:
 *                    data line encountered before #CHROM => skipping." (:469-475, :539-542)
 *   VCFXG_RS_SHORT   VCFXG_MODE_FILE: CHROM or POS missing or empty, "Warning: line has insufficient
 *                    columns => skipping." (:478-487); VCFXG_MODE_STDIN: fewer than seven tabs,
 *                    "Warning: line has <8 columns => skipping." (:544-548)
 *   VCFXG_RS_BADPOS  VCFXG_MODE_STDIN only: std::stoi of POS throws (no digits after the white space
 *                    and one sign, or a value outside int), "Warning: invalid POS => skipping."
 *                    (:552-558)
 *   VCFXG_RS_IN      CHROM's bytes equal a name and POS lies in one of its intervals: written
 *   VCFXG_RS_OUT     every other data line: dropped silently
 * VCFXG_MODE_FILE reads POS as parseIntFast does (:190-198): every digit byte of the field, the other
 * bytes skipped, accumulated modulo 2^32 and cast to int ("1e1" is 11, "-5" is 5, "abc" is 0,
 * "4294967301" is 5); eight columns are not needed.  VCFXG_MODE_STDIN reads it with std::stoi.
 * Outside the domain: an input with NUL bytes, a BED end or start of 2147483647.
 * A line whose first two (stdin mode: seven) tabs lie within its first VCFXG_RS_WINDOW bytes, or that
 * is no longer than that, is parsed by one lane; every other line by a wave (general_records counts
 * those).  rows = IN lines, warn_lines = EARLY + SHORT + BADPOS lines, data_lines = the lines that
 * are neither empty nor '#' lines, n_lines.  vcfxg_region_counts: the lines per status
 * (counts[VCFXG_RS_EMPTY .. VCFXG_RS_BADPOS]) and, in counts[7], the lines the wave path parsed.
 * vcfxg_region_filter without a table and vcfxg_region_status without a filter on this index (and
 * this table) return VCFXG_E_STATE. */
#define VCFXG_RS_EMPTY 0
#define VCFXG_RS_HEADER 1
#define VCFXG_RS_IN 2
#define VCFXG_RS_OUT 3
#define VCFXG_RS_EARLY 4
#define VCFXG_RS_SHORT 5
#define VCFXG_RS_BADPOS 6
#define VCFXG_RS_WINDOW 64
typedef struct {
    uint32_t hash_bits; /* 0: all 64 bits; 1..63: only the low bits (tests force collisions) */
} vcfxg_rs_params;
int vcfxg_regions_load(vcfxg_ctx *ctx, const char *names, const uint64_t *name_off, uint32_t n_chrom,
                       const uint32_t *chrom_id, const int32_t *start1, const int32_t *end, uint64_t n,
                       const vcfxg_rs_params *params);
int vcfxg_regions_merged(vcfxg_ctx *ctx, uint32_t *chrom_id, int32_t *start1, int32_t *end, uint64_t cap, uint64_t *n);
int vcfxg_region_filter(vcfxg_ctx *ctx, int mode, vcfxg_summary *out);
int vcfxg_region_status(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status);
int vcfxg_region_counts(const vcfxg_ctx *ctx, uint64_t counts[8]);

/* ---- VCFX_haplotype_extractor (the first segmentation, the first variable-width transpose) -------
 * Over the indexed lines (vcfxg_index from the first data line: the caller has read the header and
 * knows the n_samples names).  Lines end at '\n'; one trailing '\r' is stripped.  Per line status:
 *   VCFXG_HX_EMPTY     an empty line (VCFXG_MODE_FILE: also a line of '\r' alone), skipped
 *   VCFXG_HX_HEADER    a line that starts with '#', skipped (later "#CHROM" lines too)
 *   VCFXG_HX_SHORT     fewer than 10 fields: "Warning: skipping invalid VCF line (<10 fields)"
 *                      (VCFXG_MODE_STDIN: also a line of '\r' alone, VCFX_haplotype_extractor.cpp:739-744)
 *   VCFXG_HX_BADPOS    a byte of POS is no digit: "Warning: invalid POS => skip variant"
 *   VCFXG_HX_NOGT      FORMAT has no key that is exactly GT: dropped silently
 *   VCFXG_HX_UNPHASED  a named sample has no field, an empty GT sub-field or one without '|':
 *                      "Warning: Not all samples phased at CHROM:POS."
 *   VCFXG_HX_MEMBER    a phased variant: a member of a block
 * pos is the parsed POS (an empty POS is 0) from VCFXG_HX_NOGT up, else 0.  Members are numbered in line
 * order; member m opens a block unless it has member m - 1's CHROM bytes, pos[m] - pos[m - 1] <=
 * block_size (signed) and, with check, no sample flips (both GTs of at least 3 bytes, first and last
 * bytes a, b then c, d with a != c, b != d, a == d, b == c).  flip = the first such sample of a pair
 * that passed CHROM and distance under check, else n_samples.  Off the members member and block are
 * ~0 and flip is ~0.
 * vcfxg_haplotype_scan: statuses, POS, members, blocks, flips (rows = members, data_lines = blocks,
 * general_records = the members that are not fixed-stride -- FORMAT exactly GT and every sample "a|b" --
 * and so hold a row of the cell matrix).
 * vcfxg_haplotype_blocks: the block table and the rows' layout (rows = blocks, text_bytes = the rows'
 * bytes): row b is "CHROM\tSTART\tEND" of its first / last member, then per sample a tab and its GTs
 * joined by '|', then '\n', at row_off[b] (64-bit), row_len[b] bytes.
 * vcfxg_haplotype_text: the rows written into the context's text (vcfxg_fetch_text_range).
 * A cell of the device's matrix is VCFXG_HX_CELL_BYTES: a 32-bit offset and a 32-bit length, so no GT of
 * a line shorter than 2 GiB is too long for it.  Outside the domain: POS above 2147483647, a NUL byte. */
#define VCFXG_HX_EMPTY 0
#define VCFXG_HX_HEADER 1
#define VCFXG_HX_SHORT 2
#define VCFXG_HX_BADPOS 3
#define VCFXG_HX_NOGT 4
#define VCFXG_HX_UNPHASED 5
#define VCFXG_HX_MEMBER 6
#define VCFXG_HX_TILE_MEMBERS 32
#define VCFXG_HX_TILE_SAMPLES 64
#define VCFXG_HX_CELL_BYTES 8
typedef struct {
    int mode;            /* VCFXG_MODE_FILE / VCFXG_MODE_STDIN */
    uint32_t n_samples;  /* the names of the first "#CHROM" line (>= 1) */
    int64_t block_size;  /* -b */
    int check;           /* -c */
} vcfxg_hx_params;
int vcfxg_haplotype_scan(vcfxg_ctx *ctx, const vcfxg_hx_params *params, vcfxg_summary *out);
/* lines [first, first + count) of the last scan (any pointer may be NULL) */
int vcfxg_haplotype_lines(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status, int64_t *pos, uint64_t *member,
                          uint64_t *block, uint32_t *flip);
int vcfxg_haplotype_blocks(vcfxg_ctx *ctx, vcfxg_summary *out);
/* blocks [first, first + count) of the last vcfxg_haplotype_blocks (any pointer may be NULL) */
int vcfxg_haplotype_table(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint64_t *first_member, uint64_t *last_member,
                          int64_t *start, int64_t *end, uint64_t *row_off, uint64_t *row_len);
int vcfxg_haplotype_text(vcfxg_ctx *ctx, vcfxg_summary *out);

/* ---- VCFX_field_extractor (the first projection: records to a TSV of named cells) ---------------
 * Over the indexed lines (vcfxg_index from offset 0).  Lines end at '\n'; VCFXG_MODE_FILE strips one
 * trailing '\r' first, VCFXG_MODE_STDIN strips nothing.  Per line status:
 *   VCFXG_FX_EMPTY   an empty line, skipped
 *   VCFXG_FX_HEADER  a line that starts with '#', skipped
 *   VCFXG_FX_ROW     every other line: one row of n_cols cells
 * An output column (vcfxg_fx_col) is
 *   VCFXG_FX_STD     field `col` (0..7) of the line
 *   VCFXG_FX_INFO    the value of the INFO key (key_off, key_len: bytes of the pool).  VCFXG_MODE_FILE
 *                    (findInfoValue, VCFX_field_extractor.cpp:191-225): pairs split at ';', the key ends at
 *                    the pair's first '=', the FIRST matching pair wins, a pair without '=' is the flag "1",
 *                    an INFO of no byte or of exactly "." holds nothing.  VCFXG_MODE_STDIN (parseInfo
 *                    :538-558): an INFO whose first byte is '.' holds nothing, empty pairs are skipped, the
 *                    LAST matching pair wins.
 *   VCFXG_FX_SAMPLE  the colon token of field `col` (>= 9; 0: no such column) whose index is that of the
 *                    first FORMAT token equal to the sub-field (sub_off, sub_len).  named: col came from a
 *                    name of the first "#CHROM" line and holds only for the lines that start at or after
 *                    names_from.  VCFXG_MODE_STDIN asks INFO for the key (the whole field) first (:602).
 *   VCFXG_FX_NONE    nothing: always "."
 * A cell is VCFXG_FX_CELL_BYTES: a 32-bit offset from the line's start and a 32-bit length, or offset 0
 * and the length word VCFXG_FX_DOT (the text ".": a missing column, key, sample or sub-field, and in
 * VCFXG_MODE_FILE an empty value) or VCFXG_FX_ONE (the text "1": a flag).  A row is its cells' bytes
 * joined by tabs and a '\n'.  The matrix is line-major, one row of n_cols cells per indexed line (the
 * cells of a line that is no row are not written): one pass fills it, before the rows are numbered.
 * vcfxg_fields_load: the table; it outlives loads and indexes of the input.
 * vcfxg_fields_scan: statuses, the matrix, row numbers (the scan of the statuses) and 64-bit row offsets
 *   (the scan of the rows' bytes): rows, text_bytes; general_records = 1 when the table did not fit
 *   VCFXG_FX_TABLE_LDS bytes of LDS and was read from global memory, else 0.
 * vcfxg_fields_text: the rows written into the context's text (vcfxg_fetch_text_range), tiles of
 *   VCFXG_FX_TILE_ROWS lines through an LDS stage of VCFXG_FX_STAGE bytes.
 * Outside the domain: a NUL byte, a line of 2 GiB or more, a sample index above 2147483638. */
#define VCFXG_FX_EMPTY 0
#define VCFXG_FX_HEADER 1
#define VCFXG_FX_ROW 2
#define VCFXG_FX_STD 0
#define VCFXG_FX_INFO 1
#define VCFXG_FX_SAMPLE 2
#define VCFXG_FX_NONE 3
#define VCFXG_FX_DOT 0xFFFFFFFFu
#define VCFXG_FX_ONE 0xFFFFFFFEu
#define VCFXG_FX_NOKEY 0xFFFFFFFFu
#define VCFXG_FX_CELL_BYTES 8
#define VCFXG_FX_TABLE_LDS 16384
#define VCFXG_FX_TILE_ROWS 64
#define VCFXG_FX_STAGE 8192
typedef struct {
    uint32_t kind;             /* VCFXG_FX_STD / _INFO / _SAMPLE / _NONE */
    uint32_t col;              /* STD: 0..7; SAMPLE: the line's column (>= 9), 0: none */
    uint32_t named;            /* SAMPLE: col is a name's column */
    uint32_t key_off, key_len; /* INFO, and SAMPLE in VCFXG_MODE_STDIN; key_len VCFXG_FX_NOKEY: no key */
    uint32_t sub_off, sub_len; /* SAMPLE: the sub-field */
    uint32_t reserved;
} vcfxg_fx_col;
int vcfxg_fields_load(vcfxg_ctx *ctx, const vcfxg_fx_col *cols, uint32_t n_cols, const char *pool, uint32_t pool_bytes,
                      int mode);
int vcfxg_fields_scan(vcfxg_ctx *ctx, uint64_t names_from, vcfxg_summary *out);
/* lines [first, first + count) of the last scan (any pointer may be NULL): status, the rows before the
 * line, the text bytes before the line */
int vcfxg_fields_lines(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *status, uint64_t *row, uint64_t *row_off);
/* the matrix rows of lines [first, first + count): count * n_cols cells of two uint32_t each */
int vcfxg_fields_cells(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint32_t *cells);
int vcfxg_fields_text(vcfxg_ctx *ctx, vcfxg_summary *out);

/* ---- VCFX_haplotype_phaser (LD reuse in block phasing) ------------------
 * Over the lines from data_start (the byte after the '#CHROM' line): per line status 1 variant,
 * 4 '#' line, 3 "<10 fields", 7 invalid POS, 8 no GT in FORMAT, 0 empty (mode VCFXG_MODE_FILE:
 * phaseHaplotypesMmap / ...MmapStreaming, '\r' stripped first; VCFXG_MODE_STDIN: phaseHaplotypes
 * / ...Streaming, an empty line skipped before the strip), VCFX_haplotype_phaser.cpp:607-1259.
 * Each variant's genotypes are parseGenotypeFast codes (:312-357, the GT sub-field's allele sum,
 * -1 missing); for every variant v > 0 the device computes calculateLDFast (:366-470) of (v - 1,
 * v) over the shorter sample list -- the pair groupVariants (:1275-1322) and the streaming loops
 * test, since the block's last variant is always the previous one -- and the block rule:
 * r^2 >= threshold (and r > 0 when v's CHROM is "1").  n_samples_hint: the header's sample
 * count (the genotype row width; wider records are handled by a second pass).  rows = variants;
 * the text (vcfxg_fetch_text) holds each variant's entry "v:(CHROM:POS)" back to back. */
int vcfxg_haplotype_phaser(vcfxg_ctx *ctx, size_t data_start, int mode, double threshold, uint32_t n_samples_hint,
                           vcfxg_summary *out);
/* per variant of the last call: flags (bit 0 the pair with the previous variant passes the block
 * rule, bit 1 both have the same CHROM; 0 for variant 0), r2 (may be NULL) and the entries'
 * text offsets (n_variants + 1) */
int vcfxg_phaser_variants(vcfxg_ctx *ctx, uint8_t *flags, double *r2, uint64_t *entry_offsets);

/* ---- variant counter -------------------------------------------------------------------
 * Per line status: ROW = data line with >= 8 tab-separated columns (counted), WARN = fewer
 * columns, SKIP = empty or '#'.  strip_cr: drop a trailing '\r' first (file path).
 * Replaces countVariantsMmap / countVariants per-line work (VCFX_variant_counter.cpp:
 * 182-202, 317-389) and hasEightColumnsFast :31-44.  rows = Total Variants. */
int vcfxg_variant_count(vcfxg_ctx *ctx, int strip_cr, vcfxg_summary *out);

/* ---- K4: linkage disequilibrium ---------------------------------------------------------
 * vcfxg_ld_prepare: every data line of the indexed region with >= 10 fields and an integer
 * POS (and inside the region when has_region) becomes a variant: n_samples int8 genotype
 * codes (0/1/2, -1 missing) from each sample's GT prefix, its sums and own variance, and a
 * "CHROM\tPOS\tID" text prefix (ID "." -> "CHROM:POS" when id_dot_to_pos).  Replaces the
 * per-record parse of computeLDStreamingMmap / computeLDMatrixMmap (VCFX_ld_calculator.cpp:
 * 555-613, 697-759): fastParseInt :188-197, extractGT :177-185, parseGenotypeRaw :145-174,
 * LDVariantOpt::computeStats :243-258. */
int vcfxg_ld_prepare(vcfxg_ctx *ctx, int n_samples, int id_dot_to_pos, const char *region_chrom, size_t region_len,
                     int has_region, int region_start, int region_end, int parse_mode, uint64_t *n_variants);
/* vcfxg_index(data_start) + vcfxg_ld_prepare in one call, with the same variants, codes, sums and
 * prefixes.  For records averaging >= 512 B and n_samples <= 4096 the device walks the records
 * without a separate index sweep (one HBM pass) and synchronises with the host once; other
 * inputs take the two calls.  The context is NOT indexed afterwards (call vcfxg_index before
 * vcfxg_line_ends or a per-line call); vcfxg_ld_stream_chunk / vcfxg_ld_fetch_pairs follow as
 * after vcfxg_ld_prepare.  Replaces the same reference code as the two calls it fuses. */
int vcfxg_ld_prepare_region(vcfxg_ctx *ctx, size_t data_start, int n_samples, int id_dot_to_pos,
                            const char *region_chrom, size_t region_len, int has_region, int region_start,
                            int region_end, int parse_mode, uint64_t *n_variants);
/* parse_mode: 0 = fastParseInt POS + parseGenotypeRaw on the GT prefix (file paths, stdin
 * streaming); 1 = the stdin matrix path's std::stoi POS + parseGenotype on the whole
 * sample field (computeLD :1021-1045, parseGenotype :468-482). */
/* the variants' "CHROM\tPOS\tID" prefixes (concatenated) and M+1 offsets */
int vcfxg_ld_prefixes(vcfxg_ctx *ctx, char *text, size_t cap, uint64_t *offsets);
/* Matrix mode body: 7*M*M bytes, row-major, cell (i, j) = "\t" + r^2 text ("1.0000" on the
 * diagonal).  gate = computeRsqFast's own-variance gate (file path) vs computeRsq (stdin);
 * printf4 = setprecision(4) (stdin) vs formatR2 (file).  Replaces the matrix loops of
 * computeLDMatrixMmap :767-858 and computeLD :1050-1078. */
int vcfxg_ld_matrix(vcfxg_ctx *ctx, int gate, int printf4, uint64_t *cell_bytes);
/* Streaming-window pairs for new variants j in [j0, j1): every i with j - window <= i < j
 * (pruned when max_dist > 0 and same CHROM with |POS_j - POS_i| > max_dist), r^2 exactly as
 * computeRsqFast (:397-401 -> :352-393; int8 MFMA sums + correctly rounded fp64 epilogue),
 * kept when r^2 >= threshold, formatted as the reference's output lines (formatR2 :200-211)
 * in its order (j, then i ascending).  Text via vcfxg_fetch_text.  Replaces the window
 * loop of computeLDStreamingMmap :616-646 / computeLDStreaming :954-983. */
int vcfxg_ld_stream_chunk(vcfxg_ctx *ctx, uint64_t j0, uint64_t j1, uint64_t window, double threshold, int max_dist,
                          uint64_t *n_pairs, uint64_t *text_bytes);
/* pairs [first, first + count) of the last vcfxg_ld_stream_chunk call, in output order: variant
 * indices (i < j, into the prepared variants) and the fp64 r^2 each line's text was formatted
 * from (the value computeRsqFast returns, VCFX_ld_calculator.cpp:352-401); any pointer may be NULL */
int vcfxg_ld_fetch_pairs(vcfxg_ctx *ctx, uint64_t first, uint64_t count, uint32_t *vi, uint32_t *vj, double *r2);
/* checks the int8 MFMA operand layout the LD kernels assume (0 mismatches expected) */
int vcfxg_selftest_mfma_i8(vcfxg_ctx *ctx, int *mismatches);
/* checks the FP4 (e2m1, block-scaled) MFMA operand layout of the fast LD kernel */
int vcfxg_selftest_mfma_fp4(vcfxg_ctx *ctx, int *mismatches);

/* ---- multi-GPU shard plan (host-only, needs no device) ---------------
 * world + 1 cut offsets over the data region [lo, n) of `data`: cut i is lo + i*(n - lo)/world
 * advanced to the first line start at or after it (the reference's own split,
 * VCFX_allele_counter.cpp:889-901); shard i = [cuts[i], cuts[i+1]) holds whole records.  The
 * multi-GPU runner (vcfx_amd/shard.py, one process per GPU over torch.distributed / RCCL) hands
 * each rank its shard as a zero-copy view (VCFX_INPUT_VIEW). */
int vcfxg_shard_cuts(const char *data, size_t n, size_t lo, int world, uint64_t *cuts);

/* ---- rank cliques (SURVEY 8(b) vcfxg_shard_run's RCCL lifetime; 8(e) the count all-reduce) ----
 * A clique of n contexts, one per rank of an in-process multi-GPU run (vcfx_tool_main_sharded,
 * include/vcfx_tools.h: one host thread per rank).  On n distinct devices the reductions run
 * over RCCL (librccl loaded at run time; ncclCommInitAll + ncclAllReduce on each rank's stream,
 * over xGMI); ranks sharing a device (a rehearsal on one GPU) reduce on the host.  VCFX_RCCL=0
 * forces the host reduction; VCFX_RCCL=1 forms an RCCL clique for n = 1 too (the one-GPU check of
 * the RCCL path).  vcfxg_comm_allreduce_u64: every rank calls it from its own thread with the
 * same count (<= 64); on return vals holds the sums over all ranks (the host reduction's when the
 * status is not VCFXG_OK). */
typedef struct vcfxg_comm vcfxg_comm;
int vcfxg_comm_init(vcfxg_ctx *const *ctxs, int n, vcfxg_comm **out);
int vcfxg_comm_allreduce_u64(vcfxg_comm *comm, int rank, uint64_t *vals, size_t count);
int vcfxg_comm_uses_rccl(const vcfxg_comm *comm);
/* RCCL all-reduces run by the clique, and how many of them disagreed with the host reduction
 * every call also performs (the vote before the collective: no rank enters it unless every rank
 * staged its values; on any failure all ranks get the host sums and a non-zero status) */
int vcfxg_comm_rccl_stats(vcfxg_comm *comm, uint64_t *calls, uint64_t *mismatches);
void vcfxg_comm_destroy(vcfxg_comm *comm);

/* occurrences of `byte` in the device input's bytes [from, n) (one HBM sweep; the fused chain
 * of vcfx_pipe checks the records for '\r' with it) */
int vcfxg_count_byte(vcfxg_ctx *ctx, uint64_t from, int byte, uint64_t *count);
/* the schedule the last region call took ("af_walk", "af_walk_gt_first", "af_two_sweep", "fq_walk",
 * "fq_two_sweep", ...): a diagnostic for tests; VCFXG_SCHEDULE_LOG=path appends one line per call */
const char *vcfxg_last_schedule(const vcfxg_ctx *ctx);
/* the sample sweep of the last allele-frequency walk over GT-only records: its depth in 1 KiB
 * wave-steps (6, 8, 10 or 12; 0: no such walk yet) and, in *rolling (may be null), whether a record
 * longer than that continues rolling; chosen from the input's sample count, or forced by
 * VCFXG_AF_DEPTH (read when the context opens).  A diagnostic for tests */
int vcfxg_last_af_depth(const vcfxg_ctx *ctx, int *rolling);
/* the chunk layout of the last allele-frequency walk over GT-only records.  Returns its kind (0: no
 * such walk yet, 1 uniform, 2 fit, 3 taper, 4 split) and fills out[0..7]: a walker's bytes in the
 * full-size rounds and in the short ones, the first short dispatch round (-1: none), the blocks
 * launched, the walkers that own bytes, the resident walkers the layout was planned for (0: not
 * asked), and the taper's or split's divisor and second number.  Chosen by the plan from the region's
 * size and the resident walkers, or forced by VCFXG_WALK_LAYOUT = uniform | fit | taper:<div>:<g> |
 * split:<div>:<K1> (read when the context opens).  A diagnostic for tests */
int vcfxg_last_walk_layout(const vcfxg_ctx *ctx, int64_t out[8]);

/* device-formatted output text (without the column header line) */
int vcfxg_fetch_text(vcfxg_ctx *ctx, char *host, size_t cap);
/* bytes [offset, offset + n) of that text (outputs larger than one host buffer) */
int vcfxg_fetch_text_range(vcfxg_ctx *ctx, uint64_t offset, size_t n, void *host);
/* per-line results of the last record kernel: any pointer may be NULL */
int vcfxg_fetch_lines(vcfxg_ctx *ctx, uint64_t first, uint64_t count, int32_t *alt, int32_t *total,
                      uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
