/*
 * imcoal_fwd.h - C ABI of libimcoal_fwd.so, the MI355X (gfx950) HMM forward log-likelihood engine
 * that replaces the `ziphmm` calls behind IMCoalHMM's Forwarder / Likelihood.
 *
 * The reference has no FFI of its own for this path: it is pure Python calling the third-party
 * `ziphmm` extension module.  Each entry point below names the reference call it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes stub a maintainer would
 * put in src/IMCoalHMM/hmm.py.
 *
 * Conventions (identical to what the reference's model layer produces, model.py:44-49):
 *   all matrices row-major float64;  pi[N];  T[i*N+j] = P(next=j|cur=i) (transitions.py:241-248);
 *   E[j*S+s] = P(symbol s|state j) (emissions.py:89-100);  symbols are integers in [0,S).
 *   Every chunk (alignment file) restarts from pi and chunk log-likelihoods are summed
 *   left-to-right starting from 0.0 (likelihood.py:33).
 *   A zero-probability sequence yields -inf (not an error); NaN in -> NaN out.
 *   Limits: N <= 256 states, S <= 4096 symbols (alphabets beyond 256, e.g. the 257-symbol quartet alphabet of
 *   scripts/prepare-alignments.py:186-190, go through imc_obs_create_i32 / imc_obs_create_from_text and are kept as
 *   16-bit symbols), < 2^31 columns per chunk, and |log-likelihood| of one chunk
 *   below ~1.4e9 nats (the power-of-two exponents of a chunk are summed in int32).
 *
 * Ownership: input buffers are borrowed for the duration of the call only.  Observations are
 * copied to device memory at imc_obs_create* and owned by the library until imc_obs_free.
 * All functions return IMC_OK (0) or a negative error code; imc_last_error() gives the message
 * (thread-local).  There is NO CPU fallback: without a HIP device every compute entry point
 * fails with IMC_ERR_NODEVICE.
 *
 * Threads / processes: no HIP call is made before the first compute/create call, and the device
 * context is re-created lazily per PID, so Forwarders may be built inside multiprocessing
 * children as mcmc.py:112-121 does.  One mutex serialises the ENQUEUE of calls (plan lookup, parameter staging, kernel
 * launches); a synchronous call waits for its results without it, so other threads queue their evaluations behind it
 * (two synchronous calls on the SAME chunk list share a plan's result slots and run one after the other; a chunk is not
 * freed, and no plan released, while somebody waits on it).  The O(L) host work of imc_obs_create* (validation,
 * dictionary training, encoding) runs outside the mutex; the device encoder (imc_set_device_encoding(1),
 * imc_obs_create_device) runs on the library's stream with the mutex held.  Device ingestion (imc_set_device_ingest(1),
 * imc_obs_create_pairwise, imc_aln_open_fasta) reads its file outside the mutex and holds it for its launches.
 *
 * Environment.  csrc/options_host.hpp holds the table (imc::kOptionVars: name, field, parse rule, when it is read); this
 * list names the same set.  Read at every context creation (first library call; again after imc_set_device moves to
 * another device) unless it says otherwise:
 *   IMC_GRAPH=1        replay each plan as a hipGraph (measured: no gain)
 *   IMC_GUARD=1        test facility: every device buffer is its own virtual-memory mapping that ends flush against an
 *                      unmapped range, so any access past a buffer's end faults at once (tests/test_gpu_guard.py)
 *   IMC_BLOCKED=2..5, IMC_RANK1=0, IMC_Z4_STREAM=-1|0|1, IMC_WIDE_BLOCKED=-1|0|1   see the setters below
 *   IMC_DEVICE_ENCODE=0|1 (context creation), IMC_DEVICE_INGEST=0|1, IMC_DEVICE_TRAIN=0|1 (first use): the device
 *                      switches, consulted only while their setter has not been called
 *   A/B switches for measurements (the default is the faster setting): IMC_TABLE_PAIRS=0 (k_zpropagate4's table one
 *   dictionary depth per launch instead of two), IMC_PACK_TABLE=0 (the mat-vec chain reads the 16-padded operator
 *   table), IMC_FUSE_HEAD=0 (the parameters fetched by a k_stage_params launch and the raw operators built by k_z4_raw,
 *   instead of by the evaluation's first table launch / by each workgroup of a small launch), IMC_TABLE_SPLIT=0 (every
 *   two-depth table launch builds four tokens per wavefront; by default a launch of at most IMC_TABLE_SPLIT_MAX entries x
 *   parameter sets - four per compute unit - gives each token a wavefront and splits its products by column tile over
 *   the four MFMA blocks: same bits, shorter launches), IMC_TABLE_TRIPLES=0|1 (three dictionary depths per table launch,
 *   one wavefront per token: never / always; default: up to 12 states, where it is 2 % faster), IMC_FUSE_TAIL=0|1|2 (the
 *   chunk's last workgroup finishes the chunk instead of stitch launches: never / chunks of at most four workgroups
 *   (default) / wherever a chunk is at most 32 workgroups; 2 changes results by re-association only),
 *   IMC_XCD_AFFINE=0 (k_zpropagate4 on a plain (blocks, parameter sets) grid: by default its one-dimensional grid puts all
 *   workgroups of a parameter set on one XCD - two or four for the last B % 8 sets - so that a set's operator table is read
 *   through one L2 instead of all eight; placement only, every bit of every result is the same), IMC_CHAIN_LDS=1 (the
 *   stitch's chain step hands its vector round through LDS, not lane to lane)
 * Read at every call that uses them (tests set them between calls of one process):
 *   IMC_DEBUG=1        print the planner's cost estimates to stderr; IMC_DEBUG_LEVELS=1: of every dictionary level
 *   IMC_FORCE_LEVEL=k  pin the pair-dictionary level index (experiments; ignored if the level does not fit)
 *   IMC_DEBUG_R1=1     print where each operator segment was certified rank one (hand-off checkpoints) to stderr
 *   IMC_DICT_MIN_COUNT=n, IMC_DICT_MAX_DEPTH=d   dictionary training: occurrences a pair needs; cap on a token's depth
 *   IMC_INGEST_SLAB_BYTES   slab size of device ingestion (below); IMC_SAMPLE_TILE, IMC_SAMPLE_LDS: imcoal_sample.h
 * Read once per process, at the first call that uses it:
 *   IMC_DEBUG_HOST=1   print the host time per phase of the synchronous entry points (plan, stage, enqueue, wait)
 *                      and of chunk creation / imc_obs_recompress (copy back, training, encoding, upload)
 *
 * fork(): a child forked AFTER the parent's first imc_* call gets IMC_ERR_HIP from every call (HIP state does not
 * survive fork and nothing of the parent's is touched); fork chain processes first, or use the spawn start method.
 */
#ifndef IMCOAL_FWD_H
#define IMCOAL_FWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    IMC_OK = 0,
    IMC_ERR_ARG = -1,      /* bad shape / null pointer / unsupported size */
    IMC_ERR_SYMBOL = -2,   /* observation symbol >= nsym */
    IMC_ERR_HIP = -3,      /* HIP runtime error */
    IMC_ERR_OOM = -4,      /* host or device allocation failed */
    IMC_ERR_IO = -5,       /* cannot read / parse the observation file */
    IMC_ERR_NODEVICE = -6  /* no usable gfx950 device */
};

typedef struct imc_obs imc_obs; /* one alignment file ("chunk"), resident in HBM */

/* Library / device management ------------------------------------------------------------ */
const char *imc_version(void);
const char *imc_last_error(void);
int imc_device_count(void);          /* number of HIP devices, 0 if none (never an error) */
int imc_set_device(int device);      /* device used by subsequent calls of this process (default:
                                        the calling thread's current HIP device) */

/* Observations: replaces Forwarder.__init__, src/IMCoalHMM/hmm.py:12-16
 * (read text -> np.int32[L] -> ziphmm.preprocess_raw_observations(obs, NSYM)). -------------- */
int imc_obs_create(const uint8_t *sym, size_t L, int nsym, imc_obs **out);
int imc_obs_create_i32(const int32_t *sym, size_t L, int nsym, imc_obs **out);   /* hmm.py:14 dtype */
/* File of whitespace-separated decimal tokens, the format written by
 * scripts/prepare-alignments.py:92-105 and read at hmm.py:13-14. */
int imc_obs_create_from_text(const char *path, int nsym, imc_obs **out);   /* also accepts imc_write_cache files */
/* Where imc_obs_create_from_text turns the file into symbols.  0 (default): on the host, one thread, byte by byte
 * (csrc/obs_io.hpp), then the symbols are uploaded.  1: on the device (csrc/kernels_ingest.hpp).  The file's bytes go up
 * in slabs of at most IMC_INGEST_SLAB_BYTES (read at every call; default 4 MiB, at least 4096) through two pinned
 * staging buffers - host memory is bounded by the slab size, the file is read without the library's mutex, and slab k + 1
 * is read while slab k is on the device.  A text slab is cut after its last whitespace byte and parsed by three launches
 * (token starts and error candidates per 4096-byte tile, one scan, a scatter that writes every token's value); a cache
 * file's header is checked on the host as ever and its payload goes up packed - 2-bit payloads are unpacked by a kernel,
 * 8- and 16-bit ones are taken as they are.  The symbols are validated against nsym on the device and the chunk is built
 * from there as imc_obs_create_device builds one, so these chunks are always encoded on the device, whatever
 * imc_set_device_encoding says; the dictionary is trained where imc_set_device_training says.  Symbols, dictionaries, token streams and results
 * are those of mode 0, and so are the return code and the message of every error, in file order (an error in one slab is
 * reported before the next slab is looked at).  The device parser DECLINES a file that has a slab without any whitespace
 * or a digit run longer than 16: the host parser then reads it from its start (also what happens to anything that is
 * not a regular file).  Device memory beyond the chunk: the two slabs and, for text, one symbol buffer of the file's
 * upper bound, (bytes + 1) / 2 symbols; both are released before the token streams are encoded.
 * IMC_DEVICE_INGEST=0|1 in the environment sets the mode at start-up; any other mode is IMC_ERR_ARG. */
int imc_set_device_ingest(int mode);
/* A chunk from two aligned sequences in host memory: the pairwise rule of imc_encode_pairwise (nsym = 3) is applied on
 * the device to the bytes of the sequences, which go up through the same slabs; the chunk is the one imc_obs_create
 * builds from imc_encode_pairwise's output, and no intermediate symbols exist on the host.  IMC_ERR_ARG - before any HIP
 * call - for null pointers and L >= 2^31. */
int imc_obs_create_pairwise(const char *seq1, const char *seq2, size_t L, imc_obs **out);
/* The last chunk creation of this process: out4 = {path, bytes sent to the device as file or sequence bytes, slabs,
 * columns}; path 0 = symbols made on the host (the host parser - also for a file the device parser declined - and the
 * imc_obs_create* calls that take symbols), 1 = text parsed on the device, 2 = cache unpacked on the device,
 * 3 = pairwise rule on the device, 4 = columns from a resident alignment (imc_obs_create_from_alignment: bytes 0,
 * slabs 0).  For inspection and tests. */
int imc_last_ingest(uint64_t *out4);

/* Alignments resident on the device: the step in front of the symbols, scripts/prepare-alignments.py:66
 * (SeqIO.to_dict) and its pairwise and triplet branches (lines 77-146). ------------------------------------- */
typedef struct imc_aln imc_aln;   /* an alignment whose sequences are resident in HBM */
/* Open a FASTA file ONCE: its bytes go up in slabs of at most IMC_INGEST_SLAB_BYTES through the two pinned staging
 * buffers of device ingestion, the records are found and their line breaks squeezed out on the device
 * (csrc/kernels_align.hpp), and every record's bases end up back to back in one device buffer; the names are taken on the
 * host from the staged slab at the offsets the device reports.  No sequence exists on the host.  The result is what
 * imc_read_fasta gives for the same file.  The device parser takes lines that end in "\n" or "\r\n", '>' at column 0
 * followed by a name, sequence lines of the bytes 0x21-0x7e and empty lines anywhere; a slab may end in the middle of a
 * sequence line but not of a header line.  It DECLINES anything else - other whitespace or control bytes in a sequence
 * line, a lone '\r', whitespace in front of '>', a byte >= 0x80, an empty name, more than 4096 records, a repeated name,
 * a header line longer than a slab - and so does anything that is not a regular file: the host reader then reads the
 * file from its start and its sequences are uploaded, so every error is imc_read_fasta's.  A missing file is IMC_ERR_IO
 * before the device is asked for; without a device the call is IMC_ERR_NODEVICE.  The file is read without the library's
 * mutex; launches run on the library's stream with the mutex held.  Device memory: one buffer of the file's size (the
 * bases' size for the host reader), kept as it is - it is NOT trimmed to the bases after the parse (headers and line
 * breaks are under 2 % of a wrapped file) - plus, during the call, the two slabs and the tile tables. */
int imc_aln_open_fasta(const char *path, imc_aln **out);
/* Open a PHYLIP file ONCE, sequential (one line per record, seq-gen's output) or interleaved: the same contract, slabs,
 * staging buffers, errors and memory notes as imc_aln_open_fasta, with the parser of csrc/kernels_phylip.hpp.  The result is
 * what imc_read_phylip gives for the same file, i.e. what prepare.read_phylip defines - not the PHYLIP standard: wrapped
 * sequential records and strict 10-column names without a blank are read as that function reads them.  The host parses the
 * header line from the first slab; the device numbers the non-blank lines, keeps a table of every line's kept bytes, and
 * writes record r at r * length of a buffer of exactly n * length bytes (rounded up to 16) and the names into a table of
 * its own, so a slab may end anywhere, a name included.  The device parser takes lines that end in "\n" or "\r\n", a
 * header of two digit-only words separated and surrounded by spaces only, name lines that start at column 0 with a name
 * of the bytes 0x21-0x7e followed by nothing or by spaces and then bytes 0x21-0x7e and spaces, later lines of those bytes
 * and spaces, and empty or spaces-only lines anywhere.  It DECLINES anything else - a tab or any other control byte, a
 * lone '\r', a byte >= 0x80, a space in front of a name, a third header word, a header line that does not end inside the
 * first slab, n == 0, n > 4096, n * length larger than the file, length >= 2^31, a name of 256 bytes or more, a repeated
 * name, fewer than n name lines, a record whose bases differ in number from length, more than 2^24 non-blank lines - and
 * so does anything that is not a regular file: the host reader then reads the file from its start, so every error is
 * imc_read_phylip's.  Nothing is ever written outside the n * length bytes.  Device memory during the call, beyond the two
 * slabs and the tile tables: eight bytes per possible line (half the file's bytes, at most 2^24 lines). */
int imc_aln_open_phylip(const char *path, imc_aln **out);
int imc_aln_count(const imc_aln *aln);
const char *imc_aln_name(const imc_aln *aln, int index);          /* owned by the alignment */
size_t imc_aln_length(const imc_aln *aln, int index);
int imc_aln_sequence(const imc_aln *aln, int index, char *out, size_t capacity);   /* copy back: inspection, tests */
/* out4 = {parser: 0 host reader (declined or not a regular file), 1 device; file bytes sent; slabs; records} */
int imc_aln_info(const imc_aln *aln, uint64_t *out4);
int imc_aln_free(imc_aln *aln);                                    /* NULL is fine */
/* k = 2: pairwise rule, nsym 3; k = 3: triplet rule, nsym 65.  members[] index the alignment's records (a record may
 * occur twice).  The chunk is the one imc_obs_create builds from imc_encode_pairwise / imc_encode_triplet on the same
 * sequences: same symbols, dictionary, token streams and results, bit for bit; it keeps no reference to the alignment.
 * The symbols are made by a column kernel from the resident bases - no upload - and the chunk is built from them as
 * imc_obs_create_device builds one: encoded on the device, trained where imc_set_device_training says.  IMC_ERR_ARG -
 * before any HIP call - for null pointers, k outside {2, 3}, a member out of range, members of different lengths (the
 * message names both records and their lengths) and L >= 2^31. */
int imc_obs_create_from_alignment(const imc_aln *aln, const int *members, int k, imc_obs **out);
/* A chunk from symbols that are already in device memory (a simulated replicate, the output of another stage): d_sym
 * points to L symbols of sym_bytes = 1 (uint8), 2 (16-bit) or 4 (int32) bytes each on the library's device.  The call
 * synchronises hip_stream (a hipStream_t; NULL is the default stream), copies the symbols into a buffer of its own on
 * the device (narrowed to bytes, or to 16 bits beyond 256 symbols) and keeps no reference to d_sym.  Validation and the
 * token streams are computed on the device (csrc/kernels_encode.hpp; the tokens the host encoder would produce); only
 * when the alphabet has no dictionary yet and imc_set_device_training is 0 does the head that dictionary training looks
 * at travel to the host.
 * IMC_ERR_ARG - checked before any HIP call - for null pointers, another sym_bytes, nsym outside [1,4096], byte symbols
 * with nsym > 256 and L >= 2^31; IMC_ERR_ARG as well for a pointer that is not device memory of the library's device
 * (hipPointerGetAttributes: an error, never a fault); IMC_ERR_SYMBOL names the first column whose symbol is outside
 * [0,nsym). */
int imc_obs_create_device(const void *d_sym, size_t L, int nsym, int sym_bytes, void *hip_stream, imc_obs **out);
size_t imc_obs_length(const imc_obs *obs);
int imc_obs_nsym(const imc_obs *obs);
/* Length of the chunk's pair-compressed token stream (the `new_obs` of hmm.py:16) at the deepest
 * dictionary level whose alphabet is <= alphabet_limit; *alphabet_used gets that alphabet
 * (`new_nsyms`).  Returns the raw length when the chunk is not compressed. */
size_t imc_obs_compressed_length(const imc_obs *obs, int alphabet_limit, int *alphabet_used);
/* Joint re-compression of a data set that arrived as several chunks.  The pair dictionary of an alphabet is trained
 * by the first sufficiently long chunk created and shared by every later one (one operator table per evaluation for
 * all of them); with many chunks - 256 x 1e6 columns in BASELINE config[4] - that training sample is a single chunk
 * and the dictionary stays small (62 columns per token there, against 110+ from a 3e7-column sample).  This call
 * trains a new dictionary on a sample drawn evenly from all the given chunks, re-encodes them with it and makes it
 * the alphabet's dictionary for chunks created later.  Results change by re-association only.  Cached plans of the
 * chunks are dropped; the call synchronises the device.  Chunks too short to compress are left alone.  The
 * counterpart in the reference is ziphmm's per-Forwarder preprocessing (hmm.py:16), which compresses every file on
 * its own; imcoalhmm_amd.Likelihood calls this once for its forwarders.  The chunks must stay alive for the duration
 * of the call (do not free them from another thread meanwhile); evaluations on other threads simply wait. */
int imc_obs_recompress(imc_obs *const *chunks, int n_chunks);

/* The other two results of ziphmm.preprocess_raw_observations (hmm.py:16), at the deepest dictionary level whose
 * alphabet is <= alphabet_limit:  imc_obs_dictionary = `sym2pair` (token nsym + k is left[k] followed by right[k];
 * call with left = right = NULL to get *alphabet_used first), imc_obs_tokens = `new_obs` (copied back from the
 * device as 16-bit ids; call with tokens = NULL to get *length first).  Nothing in the reference reads them outside
 * hmm.py; they exist for inspection and tests. */
int imc_obs_dictionary(const imc_obs *obs, int alphabet_limit, uint16_t *left, uint16_t *right, size_t capacity,
                       int *alphabet_used);
int imc_obs_tokens(const imc_obs *obs, int alphabet_limit, uint16_t *tokens, size_t capacity, size_t *length,
                   int *alphabet_used);
/* Inspection sibling of imc_obs_tokens: how often every token id occurs at positions >= 1 of the stream at the
 * deepest level whose alphabet is <= alphabet_limit (the counts behind the hybrid table's hot set).  Call with
 * counts = NULL to get *alphabet_used first, then with capacity >= *alphabet_used.  Levels that keep no counts (16-bit
 * levels beyond 4096 tokens, uncompressed chunks) give zero entries. */
int imc_obs_token_counts(const imc_obs *obs, int alphabet_limit, uint32_t *counts, size_t capacity, int *alphabet_used);
int imc_obs_free(imc_obs *obs);

/* Host-side ingestion helpers (no GPU needed) -------------------------------------------- */
/* Parse a text or cache file into caller memory.  Call with sym_out = NULL to get *length first. */
int imc_read_observations(const char *path, int nsym, uint8_t *sym_out, size_t capacity, size_t *length);
/* Packed on-disk cache of a chunk: 2 bits per column when nsym <= 4 (8x smaller than the text format). */
int imc_write_cache(const char *path, const uint8_t *sym, size_t L, int nsym);
/* The pairwise symbol rule of scripts/prepare-alignments.py:99-105 on two aligned sequences:
 * 2 = either base not in ACGT (case-insensitive), 0 = equal, 1 = different. */
int imc_encode_pairwise(const char *seq1, const char *seq2, size_t L, uint8_t *sym_out);
/* Record `index` of a FASTA file read on the host (csrc/fasta_io.hpp, the C++ statement of prepare.read_fasta for ASCII
 * files): *count = records; name and sequence are copied when the pointers are non-null and the capacities suffice (name
 * NUL-terminated); *length = its bases.  Call with null buffers to size them.  IMC_ERR_IO for a file that cannot be
 * opened, a header without a name and a byte >= 0x80. */
int imc_read_fasta(const char *path, int index, char *name_out, size_t name_capacity,
                   char *seq_out, size_t seq_capacity, size_t *length, int *count);
/* The same for a PHYLIP file (csrc/phylip_io.hpp, the C++ statement of prepare.read_phylip for ASCII files: sequential or
 * interleaved, name = first word of a name line).  IMC_ERR_IO for a file that cannot be opened, a byte >= 0x80, a file
 * without a header line, a header with fewer than two words or a word that is not decimal digits only or does not fit,
 * n == 0, fewer than n name lines, a repeated name, and a record whose length differs from the header's (the message
 * names the record, its length and the header's). */
int imc_read_phylip(const char *path, int index, char *name_out, size_t name_capacity,
                    char *seq_out, size_t seq_capacity, size_t *length, int *count);
/* The triplet rule of scripts/prepare-alignments.py:134-146: i1 + 4*i2 + 16*i3 with A,C,G,T -> 0..3 (either case),
 * 64 when any of the three bases is not in ACGT.  nsym = 65. */
int imc_encode_triplet(const char *seq1, const char *seq2, const char *seq3, size_t L, uint8_t *sym_out);

/* Forward log-likelihood: replaces Forwarder.forward -> ziphmm.zip_forward,
 * src/IMCoalHMM/hmm.py:19-21, and the sum over forwarders at likelihood.py:33.
 * out_loglik[0] = sum_f log P(chunk_f | pi,T,E). */
int imc_forward(const imc_obs *const *chunks, int n_chunks, int N, int S,
                const double *pi, const double *T, const double *E, double *out_loglik);

/* B parameter sets against the same chunks in one pass (the evaluation streams of
 * genetic_algorithm.py:818-831, mcmc.py:165-174).  pis[B][N], Ts[B][N][N], Es[B][N][S];
 * out_logliks[B] (summed over chunks). */
int imc_forward_batch(const imc_obs *const *chunks, int n_chunks, int B, int N, int S,
                      const double *pis, const double *Ts, const double *Es, double *out_logliks);

/* Same, but also returns every chunk's own value: out_per_chunk[B][n_chunks]. */
int imc_forward_batch_per_chunk(const imc_obs *const *chunks, int n_chunks, int B, int N, int S,
                                const double *pis, const double *Ts, const double *Es,
                                double *out_per_chunk);

/* Multi-GPU building block: partial sums stay on the device.  d_out_partial is a DEVICE pointer
 * to B doubles, written on `hip_stream` (a hipStream_t; NULL is the DEFAULT stream, as in every HIP call - torch's
 * default stream has the handle 0 - and NOT the library's own non-blocking stream: the caller's next use of
 * d_out_partial on the stream it named is ordered behind this call, and only that).  The call returns after
 * enqueueing (no stream synchronisation: the parameters are staged through two pinned slots, so only a third call in
 * flight waits for the first one's upload).  The caller then all-reduces d_out_partial over ranks (RCCL sum).
 * Parameters are still host pointers.  Calls on one set of chunks share the plan's device buffers: a call on another
 * stream than its predecessor's (including the synchronous entry points, which use the library's stream) first waits
 * for the predecessor, so calls may move between streams; they run one after the other. */
int imc_forward_batch_device(const imc_obs *const *chunks, int n_chunks, int B, int N, int S,
                             const double *pis, const double *Ts, const double *Es,
                             double *d_out_partial, void *hip_stream);

/* One long alignment split over GPUs ("a single long file across GPUs"): every rank holds a
 * contiguous slice as its own chunk and exports the slice's STATE instead of a log-likelihood.
 *   as_operator == 0: the forward vector after the chunk, started from pi (the first slice):
 *       out_state[B][n_chunks][N], out_exp[B][n_chunks];         a_i = out_state * 2^out_exp
 *   as_operator != 0: the chunk's exact transfer operator, every column of the chunk (the first included)
 *       acting as C_o = diag(E[:,o]) T':   out_state[B][n_chunks][N][N] row-major P[i][c], out_exp[B][n_chunks][N]
 *       (one exponent per column c);                              P_ic = out_state * 2^out_exp[c]
 * The caller gathers the ranks' states (N^2 + N numbers each) and applies them in order; the log-likelihood of
 * the whole alignment is log sum_i (P_last ... P_1 a)_i.  There is no counterpart in the reference (its
 * Likelihood only sums independent files, likelihood.py:33); empty chunks are refused. */
int imc_forward_state(const imc_obs *const *chunks, int n_chunks, int as_operator, int B, int N, int S,
                      const double *pis, const double *Ts, const double *Es, double *out_state, int *out_exp);

/* Tuning / measurement ------------------------------------------------------------------ */
/* Target segment length, in stream elements (columns, or tokens on the compressed path), for the
 * parallel-in-time split (0 = automatic). */
int imc_set_segment_length(size_t columns);
/* Stream and kernel selection.
 *   1 (default): chunks are pair-compressed at creation and evaluated from the token stream whenever the
 *      operator table fits LDS for the model's N; the kernel variant is chosen from the segment/chunk ratio.
 *   0: raw symbol stream only (also skips the compression of chunks created while it is 0); kernel chosen
 *      automatically.
 *   2 / 3: as 1 but pin the kernel: 2 = one vector per lane group (k_zpropagate; N > 64: the mat-vec chain kernel
 *      k_big_vector, one segment per chunk), 3 = register-blocked operator per 16-lane row (k_zpropagate2, N <= 24;
 *      24 < N: the MFMA GEMM-chain kernels).
 *   4 / 5: as 0 but pin the kernel: 4 = k_propagate (T' in registers, LDS broadcast), 5 = k_zpropagate2. */
int imc_set_compression(int mode);
/* Forget the per-process pair dictionaries: the next sufficiently long chunk trains a new one.
 * Chunks that already exist keep the dictionary they were encoded with. */
int imc_dictionary_reset(void);
/* Where the token streams of a chunk are computed.  0 (default): on the host, one thread, one pass per merge over the
 * whole chunk (imc::encode_levels) - imc_obs_recompress first copies every raw stream back for it.  1: on the device,
 * from the symbols that are there anyway (csrc/kernels_encode.hpp): imc_obs_create* still validate and train on the
 * host; imc_obs_recompress copies back only the training heads and encodes all chunks of an alphabet in one batched run.
 * Dictionary training does not depend on this mode (imc_set_device_training), and the device encoder produces exactly the host encoder's tokens, so
 * dictionaries, streams and results are bit-identical; the mode changes set-up time only.  imc_obs_create_device always
 * encodes on the device.  IMC_DEVICE_ENCODE=0|1 in the environment sets the mode at start-up. */
int imc_set_device_encoding(int mode);
/* Where a pair dictionary is trained.  0 (default): on the host, one thread (imc::train_dictionary, csrc/pair_dict.hpp);
 * a creation whose symbols are on the device copies the head that training looks at back for it, imc_obs_recompress
 * every chunk's head.  1: on the device (csrc/kernels_train.hpp), from the symbols that are there: per byte merge one
 * count of all adjacent pairs, the winner chosen by the host's rule (largest count, then smallest pair; the depth cap
 * applies) and one replacement pass of the device encoder; per 16-bit round the counts of all distinct pairs in a table
 * in device memory, ranked on the host with the host trainer's own comparator.  The host trainer is the specification:
 * from the same symbols and the same IMC_DICT_MIN_COUNT / IMC_DICT_MAX_DEPTH the device trainer gives the same
 * dictionary entry for entry, so token streams, operator tables and results are bit-identical and the mode changes
 * set-up time only (tests/test_gpu_device_training.py; figures: profiles/README.md).  With mode 1 imc_obs_create* upload
 * the symbols before they train, imc_obs_create_device, device ingestion and imc_obs_create_pairwise copy no symbols
 * back, and neither does imc_obs_recompress while imc_set_device_encoding is 1 (the host encoder still gets the raw
 * streams it needs).  The device trainer runs on the library's stream with the mutex held.  It needs no device to be
 * set; IMC_DEVICE_TRAIN=0|1 in the environment sets the mode at start-up; any other mode is IMC_ERR_ARG. */
int imc_set_device_training(int mode);
/* The last dictionary training of this process: out4 = {path (0 host, 1 device), symbols of the sample that training
 * could look at, runs of the byte phase (1 to 3: thresholds 64, 8, 2; 0 for raw alphabets beyond 256 symbols), 16-bit
 * rounds}.  All zero before the first training.  For inspection and tests. */
int imc_last_training(uint64_t *out4);
/* Kernel timing with HIP events on the launch stream.  After imc_profile_enable(1) every
 * propagate/stitch launch is bracketed by events; imc_profile_read synchronises, returns the
 * accumulated device milliseconds and launch counts since the last reset, and resets.  ms_propagate is the
 * propagate kernel(s) of a call; k_zpropagate4's separate table launches (k_z4_raw, k_z4_level) lie in front of
 * the bracket, so the figure is the scan launch's own duration. */
int imc_profile_enable(int on);
int imc_profile_read(double *ms_propagate, double *ms_stitch, uint64_t *n_propagate, uint64_t *n_stitch);
/* Rank-one hand-off of the GEMM-chain kernels (long segments, N > 24): a segment's transfer operator is tested at a
 * fixed schedule of checkpoints (token counts, from ~8k alignment columns, each ~1.125x the previous up to ~1e5 columns,
 * then ~1.5x); at the first one
 * where every column has collapsed onto one direction (component-wise, within 2^-42) the rest of the segment
 * propagates that vector instead of the N x N operator.  The decision is taken per segment from the data of the
 * evaluation alone - no state is carried between calls, so identical calls return identical bits.  For the last
 * synchronous imc_forward* call: how many operator segments were tested and how many were certified.
 * IMC_RANK1=0 in the environment switches the hand-off off. */
int imc_last_rank1(uint64_t *checked, uint64_t *collapsed);
/* Switch the hand-off on (default) or off for plans built from now on (A/B comparisons, tests). */
int imc_set_rank1_handoff(int on);
/* Register-blocked kernel for N <= 24 (its variants do not apply to 25-32 states: see imc_set_wide_blocked): 4 (default)
 * = the fp64-MFMA scan (v_mfma_f64_4x4x4: the DP units are the same,
 * the matrix form needs a quarter of the issue slots and no cross-lane moves) with its operator table in LDS
 * (k_zpropagate3) or, where the planner's estimate says it pays, with a hybrid table - a dictionary level of up to
 * 4096 tokens in global memory / L2, the hottest operators cached in LDS (k_zpropagate4); 3 = LDS table only;
 * 5 = hybrid wherever a level beyond LDS exists (tests); 2 = k_zpropagate2, the VALU / DPP form (A/B measurements).
 * IMC_BLOCKED=2..5 in the environment selects the variant at start-up. */
int imc_set_blocked_kernel(int variant);
/* Where k_zpropagate4 takes a step's operator from: -1 (default) = automatic - STREAMED from the global table (every
 * step's operands are requested one step ahead and arrive from L1 / L2 / the Infinity Cache; nothing is cached in LDS)
 * whenever a launch holds several parameter sets (XCD-affine grid, IMC_XCD_AFFINE) or one set's table of at most 32 MB
 * (always, up to 24 states), the HYBRID form (hottest operators cached in LDS, the others streamed) otherwise;
 * 0 = always hybrid; 1 = always streamed (A/B measurements, tests).
 * IMC_Z4_STREAM=-1|0|1 in the environment sets the mode at start-up. */
int imc_set_table_streaming(int mode);
/* 25 to 32 states on the register-blocked fp64-MFMA scan (k_zpropagate4<7>: 25-28 states, <8>: 29-32): workgroups of
 * four wavefronts - one per SIMD, each with the lane's whole 512-register file - and 16 segments, the operator table
 * always streamed, built one dictionary depth per launch.  -1 (default) = automatic: in automatic mode
 * (imc_set_compression(1)) the scan is one more candidate for the token streams of a call, priced by the blocked
 * kernels' own cost model against the GEMM chain / the LDS-table vector kernels; a call that runs on the mat-vec chain
 * (many short chains) stays there.  0 = never (the kernels of the releases before this switch).  1 = wherever every
 * dictionary of the call has a token level the scan can run (a table the streamed form accepts, see
 * imc_set_table_streaming).  Raw streams, chunks too short to be compressed and the pinned modes 2-5 of
 * imc_set_compression keep their kernels whatever the mode.
 * IMC_WIDE_BLOCKED=-1|0|1 in the environment sets the mode at start-up. */
int imc_set_wide_blocked(int mode);
/* Description of the last launch plan, out8[0..7] = segments, vectors, per-column segment length,
 * executed vector-columns (per-column kernel), token segment length, executed vector-tokens (token
 * kernel), tokens in the compressed streams, token alphabet. */
int imc_last_plan(uint64_t *out8);
/* Propagate kernels launched by the last forward call, '+'-joined, e.g. "k_zpropagate2<5>[tokens]". */
const char *imc_last_kernels(void);

#ifdef __cplusplus
}
#endif
#endif /* IMCOAL_FWD_H */
