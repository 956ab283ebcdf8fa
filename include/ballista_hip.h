/*
 * ballista_hip.h — C ABI of libballista_hip.so, the MI355X-native physical execution layer
 * that drops in underneath a Ballista executor.
 *
 * What it replaces.  A Ballista executor runs one call per task,
 *     partition.plan.execute(part)          rust/executor/src/flight_service.rs:117-121
 * on a tree of DataFusion operators rebuilt from the wire plan
 *     rust/core/src/serde/physical_plan/from_proto.rs:58-346  (operators)
 *     rust/core/src/serde/physical_plan/from_proto.rs:348-364 (compile_expr)
 * and drains the resulting RecordBatchStream (rust/core/src/utils.rs:49-84).  The trait it
 * calls through is DataFusion's `ExecutionPlan` as visible in the reference's own
 * implementations (rust/core/src/execution_plans/query_stage.rs:49-85):
 *     schema(), output_partitioning(), children(), with_new_children(), execute(partition)
 * and `RecordBatchStream` (rust/core/src/memory_stream.rs:57-92).  Every entry point below
 * names the reference interface it stands in for.  A Rust `GpuExec: ExecutionPlan` shim binds
 * these with `extern "C"` (INTEGRATION.md shows the binding).
 *
 * Conventions:
 *   - every function returns a bhip_status; 0 = OK.  Nothing aborts or throws across the ABI;
 *     the message of the last failure on the calling thread is bhip_last_error().
 *   - BHIP_ENOTIMPL means "this plan/expression/type is outside the GPU path": the caller keeps
 *     its CPU operator for that subtree (there is NO CPU fallback inside this library).
 *   - handles are reference counted and immutable after creation; plans may be shared between
 *     threads and executed concurrently (the executor runs `concurrent_tasks` tasks at once,
 *     rust/executor/executor_config_spec.toml:57-62); a stream is single-consumer.
 *   - batches cross the boundary as Arrow C Data Interface structs (host memory) or stay
 *     device-resident (bhip_batch) between chained GPU operators.
 *   - strings are UTF-8, NUL terminated, and are copied; arrays are copied.
 */
#ifndef BALLISTA_HIP_H
#define BALLISTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Arrow C Data / C Stream interface (https://arrow.apache.org/docs/format/CDataInterface.html) */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
    const char* format;
    const char* name;
    const char* metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema** children;
    struct ArrowSchema* dictionary;
    void (*release)(struct ArrowSchema*);
    void* private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void** buffers;
    struct ArrowArray** children;
    struct ArrowArray* dictionary;
    void (*release)(struct ArrowArray*);
    void* private_data;
};
#endif
#ifndef ARROW_C_STREAM_INTERFACE
#define ARROW_C_STREAM_INTERFACE
struct ArrowArrayStream {
    int (*get_schema)(struct ArrowArrayStream*, struct ArrowSchema* out);
    int (*get_next)(struct ArrowArrayStream*, struct ArrowArray* out);
    const char* (*get_last_error)(struct ArrowArrayStream*);
    void (*release)(struct ArrowArrayStream*);
    void* private_data;
};
#endif

/* ---- status ---------------------------------------------------------------------------
 * mirrors the error kinds the executor maps to tonic::Status::internal
 * (rust/executor/src/flight_service.rs:344-354; rust/core/src/error.rs:30-163) */
typedef int32_t bhip_status;
enum {
    BHIP_OK = 0,
    BHIP_EINVAL = 1,     /* DataFusionError::Plan / Internal: malformed plan, unknown column, type mismatch */
    BHIP_ENOTIMPL = 2,   /* DataFusionError::NotImplemented: keep the CPU operator */
    BHIP_EEXEC = 3,      /* DataFusionError::Execution / ArrowError: e.g. "Divide by zero error" */
    BHIP_EHIP = 4,       /* a HIP runtime call failed (message carries hipGetErrorString) */
    BHIP_EOOM = 5        /* device allocation failed */
};
const char* bhip_last_error(void);
const char* bhip_version(void);

/* ---- types (Arrow types of the TPC-H schemas, rust/benchmarks/tpch/src/main.rs:267-360) */
typedef enum {
    BHIP_INT32 = 1, BHIP_INT64 = 2, BHIP_UINT8 = 3, BHIP_UINT64 = 4, BHIP_FLOAT64 = 5,
    BHIP_DATE32 = 6, BHIP_BOOLEAN = 7, BHIP_UTF8 = 8,
    /* the other primitive types of the serde (rust/core/proto/ballista.proto:755-790) */
    BHIP_INT8 = 9, BHIP_INT16 = 10, BHIP_UINT16 = 11, BHIP_UINT32 = 12, BHIP_FLOAT32 = 13, BHIP_DATE64 = 14,
    BHIP_TIMESTAMP_S = 15, BHIP_TIMESTAMP_MS = 16, BHIP_TIMESTAMP_US = 17, BHIP_TIMESTAMP_NS = 18,
    /* schemas only: a Utf8 column whose Arrow / IPC form is LargeUtf8 (64-bit offsets); on the device it is BHIP_UTF8 */
    BHIP_LARGE_UTF8 = 19,
    /* schemas only: variable-length bytes (the digests of sha224 .. sha512) in the buffer layout of BHIP_UTF8 */
    BHIP_BINARY = 20
} bhip_dtype;

typedef struct bhip_ctx bhip_ctx;        /* one GPU: allocator, stream pool */
typedef struct bhip_batch bhip_batch;    /* device-resident RecordBatch */
typedef struct bhip_plan bhip_plan;      /* Arc<dyn ExecutionPlan> */
typedef struct bhip_stream bhip_stream;  /* Pin<Box<dyn RecordBatchStream>> */

/* ---- context ------------------------------------------------------------------------------ */
bhip_status bhip_ctx_create(int device, bhip_ctx** out);
void bhip_ctx_release(bhip_ctx* ctx);
bhip_status bhip_ctx_synchronize(bhip_ctx* ctx);
/* bytes currently held / high-water mark of the context's device allocator */
bhip_status bhip_ctx_memory(bhip_ctx* ctx, uint64_t* in_use, uint64_t* peak);

/* ---- batches ------------------------------------------------------------------------------
 * RecordBatch (columns are immutable, shared buffers).  Host constructors copy to the device;
 * bhip_batch_from_device adopts device pointers without copying (caller keeps them alive and
 * unchanged until the batch is released).  Layout per column = Arrow: fixed-width values, or
 * Utf8 int32 offsets (length+1) + bytes, Boolean = bitmap; validity bitmap optional (NULL =
 * no nulls); offset must be 0 for device columns.
 *
 * Device columns are read where they lie, so bhip_batch_from_device asks of each buffer:
 *   alignment   values: the value's own width (1, 2, 4 or 8 bytes); Utf8 offsets: 4 bytes; Utf8 bytes: none;
 *               validity bitmaps and Boolean values: 8 bytes.  A pointer that breaks it -> BHIP_EINVAL.
 *               (Buffers on a 16-byte boundary take the wide-load kernels; any other placement gives the same
 *               results through the general ones.)
 *   extent      the library reads a bitmap up to the end of the 64-bit word that holds its last bit — the caller
 *               provides ((n_rows + 63) / 64) * 8 readable bytes; the bits past n_rows may hold anything.
 *               1- and 2-byte values are read as 4-byte words counted from the buffer's first byte (wherever that
 *               lies), up to the end of the word that holds the last value: the caller provides
 *               ((n_rows * width + 3) / 4) * 4 readable bytes; the bytes past the last value may hold anything.
 *               Nothing else is read beyond the Arrow sizes: n_rows * width bytes of 4- and 8-byte values,
 *               (n_rows + 1) * 4 bytes of offsets, data_bytes bytes of Utf8 values. */
typedef struct {
    const char* name;
    int32_t dtype;            /* bhip_dtype */
    int32_t nullable;         /* schema nullability */
    const void* data;         /* values | Utf8 bytes | Boolean bitmap */
    const int32_t* offsets;   /* Utf8 only */
    const uint8_t* validity;  /* Arrow validity bitmap or NULL */
    int64_t data_bytes;       /* Utf8: number of value bytes; else ignored */
} bhip_column_desc;

bhip_status bhip_batch_from_host(bhip_ctx* ctx, int32_t n_cols, const bhip_column_desc* cols, int64_t n_rows,
                                 bhip_batch** out);
bhip_status bhip_batch_from_device(bhip_ctx* ctx, int32_t n_cols, const bhip_column_desc* cols, int64_t n_rows,
                                   bhip_batch** out);
/* Scan leaf for TPC-H `.tbl` text — where the reference has CsvExec(delimiter '|', no header, explicit schema):
 * rust/benchmarks/tpch/src/main.rs:129-150, rust/core/src/serde/physical_plan/from_proto.rs:93-110.
 * `text` (host memory, < 4 GiB, whole lines) is copied to the device once; lines, fields and values are found
 * there.  A file of any size goes through bhip_plan_text_scan, which streams it in slabs.  fields[i].name / .dtype / .nullable describe the file's fields in order (data pointers unused);
 * `projection` = indices of the fields to materialise, in output order (NULL: all).  Int32, Int64, Float64
 * ([-]digits[.digits], converted exactly), Date32 (YYYY-MM-DD) and Utf8 columns.  Malformed text -> BHIP_EEXEC;
 * decimals beyond 15 significant digits or other column types -> BHIP_ENOTIMPL (keep the CPU reader). */
bhip_status bhip_batch_from_tbl(bhip_ctx* ctx, const void* text, int64_t n_bytes, int32_t n_fields,
                                const bhip_column_desc* fields, int32_t n_projection, const int32_t* projection,
                                bhip_batch** out);
/* Scan leaf for general CSV text — where the reference has CsvExec with the `has_header` and `delimiter` of the wire
 * plan (`--format csv`: CsvReadOptions::new().schema(..).has_header(true), rust/benchmarks/tpch/src/main.rs:129-150).
 * Arguments as for bhip_batch_from_tbl, plus `opts` (NULL: ',' and a header).  Accepted text: fields separated by
 * `delimiter` (one byte, not '"', '\n' or '\r': else BHIP_EINVAL); records ended by '\n' or '\r\n' outside quotes,
 * the last one may be unterminated; with `has_header` the first record is skipped (it is not compared with the
 * schema).  A field whose first byte is '"' runs to the matching '"'; inside it "" is one '"', and delimiter, '\r'
 * and '\n' are data.  Values as for `.tbl`, plus Boolean (true / false in any letter case).  An empty field
 * (unquoted, or "") of a column that is not Utf8 is NULL when fields[i].nullable, BHIP_EEXEC when not; of a Utf8
 * column it is the empty string.  A column in which no NULL occurred carries no validity buffer.  Fewer fields than
 * the schema, a blank line, a malformed value -> BHIP_EEXEC.  A '"' inside an unquoted field, bytes between a
 * closing quote and the next delimiter, a '\r' that is not part of a record end, an unclosed quote: CSV readers
 * disagree on these -> BHIP_ENOTIMPL (keep the CPU reader).  Text < 4 GiB per call; a file of any size goes through
 * bhip_plan_text_scan. */
typedef struct bhip_csv_opts {
    uint8_t delimiter;        /* e.g. ',' */
    int32_t has_header;       /* != 0: the first record holds column names */
} bhip_csv_opts;
bhip_status bhip_batch_from_csv(bhip_ctx* ctx, const void* text, int64_t n_bytes, int32_t n_fields,
                                const bhip_column_desc* fields, int32_t n_projection, const int32_t* projection,
                                const bhip_csv_opts* opts, bhip_batch** out);
/* Arrow C Data Interface: `array` is a struct array (one child per column) as produced by
 * RecordBatch export; it is consumed (released) on success. */
bhip_status bhip_batch_import_arrow(bhip_ctx* ctx, struct ArrowArray* array, struct ArrowSchema* schema,
                                    bhip_batch** out);
/* copies the batch to host memory and exports it; the caller releases out_array/out_schema. */
bhip_status bhip_batch_export_arrow(bhip_batch* batch, struct ArrowArray* out_array, struct ArrowSchema* out_schema);
void bhip_batch_retain(bhip_batch* batch);
void bhip_batch_release(bhip_batch* batch);
int64_t bhip_batch_num_rows(const bhip_batch* batch);
int32_t bhip_batch_num_columns(const bhip_batch* batch);
/* column metadata; `name` stays valid while the batch lives */
bhip_status bhip_batch_column_info(const bhip_batch* batch, int32_t i, const char** name, int32_t* dtype,
                                   int32_t* nullable, int64_t* data_bytes, int32_t* has_validity);
/* raw device pointers of column i (for zero-copy consumers, e.g. an RCCL exchange) */
bhip_status bhip_batch_column_device(const bhip_batch* batch, int32_t i, const void** data, const int32_t** offsets,
                                     const uint8_t** validity);
/* copy column i to caller-provided host buffers (any of the three may be NULL) */
bhip_status bhip_batch_column_to_host(const bhip_batch* batch, int32_t i, void* data, int32_t* offsets, uint8_t* validity);
/* ArrayRef::get_array_memory_size summed over columns — the num_bytes of PartitionStats
 * (rust/core/src/utils.rs:60-83) */
int64_t bhip_batch_memory_size(const bhip_batch* batch);

/* ---- physical expressions ---------------------------------------------------------------
 * A flat POSTFIX program of nodes mirroring the expression kinds the physical-plan serde can
 * ship (rust/core/src/serde/physical_plan/to_proto.rs:380-511; LogicalExprNode,
 * rust/core/proto/ballista.proto:14-45).  Binary operators are named by the wire strings of
 * rust/core/src/serde/logical_plan/from_proto.rs:937-957 ("And" "Or" "Eq" "NotEq" "LtEq" "Lt"
 * "Gt" "GtEq" "Plus" "Minus" "Multiply" "Divide" "Like" "NotLike"). */
typedef enum {
    BHIP_EXPR_COLUMN = 1,      /* name                                  pushes 1            */
    BHIP_EXPR_LITERAL = 2,     /* dtype + value (is_null: typed NULL)   pushes 1            */
    BHIP_EXPR_BINARY = 3,      /* op ; pops right, left                                     */
    BHIP_EXPR_CAST = 4,        /* dtype ; pops 1                                            */
    BHIP_EXPR_NOT = 5,
    BHIP_EXPR_IS_NULL = 6,
    BHIP_EXPR_IS_NOT_NULL = 7,
    BHIP_EXPR_NEGATIVE = 8,
    BHIP_EXPR_IN_LIST = 9,     /* n_args list items + 1 ; negated       pops n_args+1       */
    BHIP_EXPR_CASE = 10,       /* n_args = #when/then pairs; flags bit0: has base expr,
                                  bit1: has else.  Stack order: [base] w1 t1 ... wn tn [else] */
    BHIP_EXPR_SCALAR_FN = 11   /* name = function ; pops n_args, pushed in order.  One argument: sqrt abs floor ceil round
                                  trunc signum exp ln log2 log10 sin cos tan asin acos atan, lower upper trim ltrim rtrim,
                                  octet_length, sha224 sha256 sha384 sha512, to_timestamp.  Two: nullif(a, b),
                                  date_trunc('granularity', t), left(s, n), right(s, n), strpos(s, sub), starts_with(s, prefix),
                                  date_part('part', x).  Two or three: substr(s, start[, count]) (alias substring).  One to
                                  eight: concat.  char_length (aliases length, character_length) takes one.  n, start and count
                                  are Int64.  md5 and array: BHIP_ENOTIMPL */
} bhip_expr_kind;

typedef struct {
    int32_t kind;            /* bhip_expr_kind */
    int32_t dtype;           /* LITERAL / CAST */
    int32_t n_args;
    int32_t flags;           /* LITERAL: bit0 = is_null ; IN_LIST: bit0 = negated ; CASE: see above */
    const char* name;        /* COLUMN name / BINARY operator / SCALAR_FN name / Utf8 literal */
    int64_t i64;             /* integer, Date32, Boolean literal */
    double f64;              /* Float64 literal */
} bhip_expr_node;

typedef struct {
    const bhip_expr_node* nodes;
    int32_t n_nodes;
} bhip_expr;

/* AggregateExpr (to_proto.rs:348-378: Sum / Avg / Count are what the serde ships; Min / Max are
 * accepted too) */
/* COUNT / SUM / AVG (DISTINCT x): the function over the distinct non-NULL values of x in the group.  BHIP_AGG_SINGLE only (the
 * state is a set, not a fixed-width column: BHIP_ENOTIMPL in PARTIAL / FINAL); no wire form.  Two values are the same value when
 * a GROUP BY on wide keys would put them into one group: fixed-width types by their bits (-0.0 and +0.0, NaNs of different payloads
 * are different values), Utf8 by length and bytes ("" is a value, NULL is none), Boolean by its bit.  COUNT_DISTINCT takes every
 * type a group key can have, SUM_DISTINCT / AVG_DISTINCT what SUM / AVG take.  One operator may mix plain aggregates with DISTINCT
 * ones over up to 8 different argument expressions (arguments that print alike count once), with at most 15 group expressions;
 * neither those arguments nor the group expressions beside them may hold a string-valued function (lower(s), CAST(x AS Utf8) ...:
 * BHIP_ENOTIMPL), plain Utf8 columns may stand in both places; input column names __distinct_0 .. are reserved (BHIP_EINVAL). */
typedef enum {
    BHIP_AGG_SUM = 1, BHIP_AGG_AVG = 2, BHIP_AGG_COUNT = 3, BHIP_AGG_MIN = 4, BHIP_AGG_MAX = 5,
    BHIP_AGG_COUNT_DISTINCT = 6, BHIP_AGG_SUM_DISTINCT = 7, BHIP_AGG_AVG_DISTINCT = 8
} bhip_agg_fn;
typedef struct {
    int32_t fn;              /* bhip_agg_fn */
    bhip_expr arg;
    const char* name;        /* output field name */
} bhip_aggregate;

/* PhysicalSortExpr (ballista.proto PhysicalSortExprNode) */
typedef struct {
    bhip_expr expr;
    int32_t descending;
    int32_t nulls_first;
} bhip_sort_expr;

/* PARTIAL / FINAL: from_proto.rs:181-184.  SINGLE (no wire form): raw rows in, final values out, in one operator — the output
 * schema of FINAL over PARTIAL with the same expressions (COUNT / COUNT_DISTINCT UInt64 not nullable, SUM_DISTINCT the SUM type,
 * AVG_DISTINCT Float64, both nullable); legal for every function.  execute(p) aggregates input partition p alone and the output
 * partitioning is the input's, so the constructor takes the mode only when every group lies in one partition: the input has one
 * partition, or it is Hash-partitioned on expressions that are all among the group expressions (compared as printed) and there is
 * a group expression; otherwise BHIP_EINVAL, naming the MergeExec or RepartitionExec(Hash ...) to put under it. */
typedef enum { BHIP_AGG_PARTIAL = 0, BHIP_AGG_FINAL = 1, BHIP_AGG_SINGLE = 2 } bhip_agg_mode;
/* HashJoinExec join types; left is the build side.  0-2 are the wire values of from_proto.rs:268-272; FULL / SEMI / ANTI carry the
   wire values of the JoinType enum that followed it (3, 4, 5) and decode from a plan; RIGHT_SEMI / RIGHT_ANTI have no wire value
   and are reached through bhip_plan_hash_join only.  SEMI / ANTI: the left rows with / without a partner, left fields only;
   RIGHT_SEMI / RIGHT_ANTI: the right rows, right fields only.  NULL keys never match (ANTI emits the rows that have one). */
typedef enum {
    BHIP_JOIN_INNER = 0, BHIP_JOIN_LEFT = 1, BHIP_JOIN_RIGHT = 2, BHIP_JOIN_FULL = 3, BHIP_JOIN_SEMI = 4, BHIP_JOIN_ANTI = 5,
    BHIP_JOIN_RIGHT_SEMI = 6, BHIP_JOIN_RIGHT_ANTI = 7
} bhip_join_type;
typedef enum {                                                                /* from_proto.rs:143-158 */
    BHIP_PART_UNKNOWN = 0, BHIP_PART_ROUND_ROBIN = 1, BHIP_PART_HASH = 2
} bhip_partitioning;

/* ---- plans: one constructor per operator the serde can build (from_proto.rs line cited) ----
 * Constructors take a reference on their inputs; the caller still releases its own. */
/* leaf: in-memory partitions (datafusion MemoryExec; stands in for CsvExec/ParquetExec
 * :93-121 and ShuffleReaderExec :277-286 whose decoding stays on the host side).
 * batches[offsets[p] .. offsets[p+1]) are the batches of partition p. */
bhip_status bhip_plan_memory(bhip_ctx* ctx, int32_t n_partitions, const int32_t* offsets, bhip_batch* const* batches,
                             bhip_plan** out);
/* EmptyExec :287-290 — schema given as column descs with NULL data */
/* leaf over a host-side Arrow C stream — the C image of a CPU child operator's RecordBatchStream
 * (rust/core/src/memory_stream.rs:57-92): the stream is MOVED into the plan, drained on the first execute (each batch
 * imported to the device) and replayed on later executes.  One output partition. */
bhip_status bhip_plan_arrow_stream(bhip_ctx* ctx, struct ArrowArrayStream* stream, bhip_plan** out);
/* the same with one stream per output partition of the CPU child (all moved into the plan): partition p of the leaf is
 * streams[p]; a join above drains every partition of its build side, as the reference's collect-left join does */
bhip_status bhip_plan_arrow_streams(bhip_ctx* ctx, int32_t n_partitions, struct ArrowArrayStream* const* streams, bhip_plan** out);
/* ParquetExec::try_from_files(filenames, projection, None, batch_size, num_partitions)  :111-121 — the files are dealt out to
 * `num_partitions` output partitions in chunks; one batch per row group.  projection NULL: every column.  Pages are located
 * and decompressed (Snappy) on the host, values are decoded on the device (dictionary runs, NULL re-insertion, gathers).
 * Flat schemas of INT32 / INT64 / DOUBLE / BOOLEAN / BYTE_ARRAY (+ DATE), PLAIN and RLE_DICTIONARY, data pages V1 / V2,
 * UNCOMPRESSED / SNAPPY; anything else is BHIP_ENOTIMPL. */
bhip_status bhip_plan_parquet(bhip_ctx* ctx, int32_t n_files, const char* const* paths, int32_t n_projection, const uint32_t* projection,
                              int32_t num_partitions, bhip_plan** out);
/* CsvExec on the device over files of any size (CsvExec::try_new(path, options, projection, batch_size), from_proto.rs:93-110):
 * one partition per file, each file streamed through the `.tbl` scan (BHIP_TEXT_TBL: bhip_batch_from_tbl's grammar) or the CSV
 * scan (BHIP_TEXT_CSV: bhip_batch_from_csv's, with `csv`) in slabs of `slab_bytes` of text, ONE BATCH PER SLAB: a reader thread
 * fills pinned host buffers while the slab before crosses PCIe and the one before that is parsed.  A slab is cut wherever its
 * bytes end; the records that end in it form its batch and the rest is carried to the next slab on the device.  Concatenated,
 * the batches are what the one-shot call gives on the whole text.  slab_bytes: a multiple of 16 KiB in [16 KiB, 2 GiB], or 0 for
 * the environment's BHIP_TEXT_SLAB_MB (MiB, fractions allowed), else 64 MiB; anything else is BHIP_EINVAL.  The one limit: a
 * record must fit one slab — a record that does not end within the carry (one slab at most) plus one slab, i.e. not in the
 * slab it starts in nor in the next one (or a quote that is never closed), is BHIP_ENOTIMPL.  Errors surface at the bhip_stream_next that parses the offending slab, with the file name and the byte offset
 * of the slab's start; batches before it have been delivered.  The reference's reader cuts batches by rows (batch_size); this
 * one cuts by bytes of text.  opts NULL: `.tbl`, default slab. */
#define BHIP_TEXT_TBL 0
#define BHIP_TEXT_CSV 1
typedef struct bhip_text_scan_opts {
    int32_t format;        /* BHIP_TEXT_TBL | BHIP_TEXT_CSV */
    bhip_csv_opts csv;     /* CSV only */
    int64_t slab_bytes;    /* 0: default / BHIP_TEXT_SLAB_MB */
} bhip_text_scan_opts;
bhip_status bhip_plan_text_scan(bhip_ctx* ctx, int32_t n_files, const char* const* paths, int32_t n_fields,
                                const bhip_column_desc* fields, int32_t n_projection, const int32_t* projection,
                                const bhip_text_scan_opts* opts, bhip_plan** out);
bhip_status bhip_plan_empty(bhip_ctx* ctx, int32_t n_cols, const bhip_column_desc* schema, int32_t produce_one_row,
                            bhip_plan** out);
bhip_status bhip_plan_filter(bhip_plan* input, const bhip_expr* predicate, bhip_plan** out);          /* :81-92  */
bhip_status bhip_plan_projection(bhip_plan* input, int32_t n, const bhip_expr* exprs, const char* const* names,
                                 bhip_plan** out);                                                   /* :69-80  */
bhip_status bhip_plan_hash_aggregate(bhip_plan* input, int32_t mode, int32_t n_group, const bhip_expr* group_exprs,
                                     const char* const* group_names, int32_t n_aggr, const bhip_aggregate* aggr,
                                     bhip_plan** out);                                               /* :173-252 */
bhip_status bhip_plan_hash_join(bhip_plan* left, bhip_plan* right, int32_t n_on, const char* const* left_keys,
                                const char* const* right_keys, int32_t join_type, bhip_plan** out);  /* :253-276 */
/* the same with a residual join filter: a left and a right row are partners when their keys are equal AND `filter` is TRUE (NULL
 * is not a match), for every join type — a row all of whose key-equal candidates fail it is a row without a partner.  The filter is
 * typed against the INNER join's output schema of the two children whatever the join type (left fields, then right fields minus a
 * right key column named like its left partner); with a filter, a non-key name on both sides is BHIP_EINVAL for SEMI / ANTI /
 * RIGHT_SEMI / RIGHT_ANTI as well; a filter that reads no column is BHIP_ENOTIMPL.  Output schema and nullability are those of bhip_plan_hash_join.  filter NULL: exactly
 * bhip_plan_hash_join.  No wire form (HashJoinExecNode has no field for it). */
bhip_status bhip_plan_hash_join_filter(bhip_plan* left, bhip_plan* right, int32_t n_on, const char* const* left_keys,
                                       const char* const* right_keys, int32_t join_type, const bhip_expr* filter, bhip_plan** out);
/* NestedLoopJoinExec: the join without an equality key (a range or band predicate, a cross product, a one-row subquery).  left is the
 * build side, collected whole; right the probe side, one output stream per right partition.  A left and a right row are partners when
 * `filter` is TRUE (NULL is not a match); filter NULL: every pair (the cross join).  All eight bhip_join_type values, with the meaning
 * and the nullability they have in bhip_plan_hash_join; output schema: the left fields then the right fields (SEMI / ANTI: left only,
 * RIGHT_SEMI / RIGHT_ANTI: right only); two output columns of one name are BHIP_EINVAL.  The filter is typed against the INNER output
 * schema whatever the join type (so with a filter a name on both sides is BHIP_EINVAL for the existence types too); one that reads no
 * column is BHIP_ENOTIMPL.  LEFT / FULL / SEMI / ANTI need a right child of one partition (BHIP_ENOTIMPL otherwise: MergeExec).
 * No wire form (the reference's PhysicalPlanNode has no such node): this entry point only. */
bhip_status bhip_plan_nested_loop_join(bhip_plan* left, bhip_plan* right, int32_t join_type, const bhip_expr* filter /* NULL: cross */,
                                       bhip_plan** out);
bhip_status bhip_plan_sort(bhip_plan* input, int32_t n, const bhip_sort_expr* exprs, bhip_plan** out); /* :291-331 */
/* WindowAggExec: ONE window specification — PARTITION BY partition_by ORDER BY order_by — and the functions over it; different
 * specifications are stacked operators.  The operator sorts its input itself (a single input partition, like SortExec: put a MergeExec
 * below it otherwise) by the partition keys ASC NULLS FIRST and then the order keys as given, with SortExec's stable sort, and the
 * rows leave in that order in one batch: the input's fields followed by one field per window expression.  Two rows are in one
 * partition when every partition key is equal and peers when every order key is equal as well — NULL equals NULL, floats by bit
 * pattern, Utf8 by bytes (the GROUP BY rule).  At most 8 partition keys and 8 order keys (BHIP_ENOTIMPL beyond).
 *   ROW_NUMBER, RANK, DENSE_RANK   no argument; UInt64, not nullable (RANK / DENSE_RANK without order_by: 1 on every row)
 *   LAG(x, k), LEAD(x, k)          x: any fixed-width type, Boolean, Utf8; k = `offset` >= 0 rows; the type of x, nullable: NULL
 *                                  where row i -/+ k lies outside the partition (no default value)
 *   FIRST_VALUE(x), LAST_VALUE(x)  the type of x; the FRAME's first row (of a named frame: the partition's first row) / last row;
 *                                  nullable like x, and always under a rows frame that can be empty (start > 0 or end < 0)
 *   SUM, AVG, COUNT, MIN, MAX      over the frame, with the result types and NULL rules of a Final HashAggregateExec: SUM of signed /
 *                                  unsigned integers Int64 / UInt64 (wrapping), floating SUM and every AVG Float64, COUNT UInt64 and
 *                                  never NULL, MIN / MAX the type of x (NaN skipped unless nothing else is there); NULL when the frame
 *                                  holds no non-NULL value.  MIN / MAX over Utf8 or Boolean: BHIP_ENOTIMPL.  COUNT(*) = COUNT of a
 *                                  UInt8 literal 1.
 * Frames (the aggregates and LAST_VALUE; ignored elsewhere): PARTITION = the whole partition; ROWS_TO_CURRENT = UNBOUNDED PRECEDING
 * .. CURRENT ROW; RANGE_TO_CURRENT = UNBOUNDED PRECEDING .. the last peer of the current row; DEFAULT = SQL's: RANGE_TO_CURRENT with
 * an order_by, PARTITION without one (resolved when the plan is made).
 * Sliding ROWS frames come beside these structs, through bhip_plan_window_frames: for row i of the partition [ps, pe] the frame is rows
 * max(ps, i + start) .. min(pe, i + end) in the operator's order (an unbounded side: ps / pe), any Int64 offsets; start > end (both
 * finite) is BHIP_EINVAL.  An empty frame gives COUNT 0 and NULL elsewhere.  UNBOUNDED PRECEDING .. CURRENT ROW and .. UNBOUNDED
 * FOLLOWING are ROWS_TO_CURRENT and PARTITION; on a function without a frame (ranking, LAG, LEAD) a rows frame is ignored.  With two
 * finite ends the floating SUM and every AVG add the frame's non-NULL values in row order to +0.0 in Float64 (bit-reproducible), and
 * these two, MIN and MAX take at most 4096 rows of frame (BHIP_ENOTIMPL beyond); the same four over k .. UNBOUNDED FOLLOWING with a
 * finite k are BHIP_ENOTIMPL.  COUNT, the integer SUM, FIRST_VALUE and LAST_VALUE take every frame.
 * RANGE and GROUPS frames with offsets come through bhip_plan_window_frame_specs (below).  EXCLUDE, NTILE, PERCENT_RANK, CUME_DIST,
 * NTH_VALUE and IGNORE NULLS are not there.  No wire form (the reference's PhysicalPlanNode has no window node). */
typedef enum {
    BHIP_WIN_ROW_NUMBER = 1, BHIP_WIN_RANK = 2, BHIP_WIN_DENSE_RANK = 3, BHIP_WIN_LAG = 4, BHIP_WIN_LEAD = 5, BHIP_WIN_FIRST_VALUE = 6,
    BHIP_WIN_LAST_VALUE = 7, BHIP_WIN_SUM = 8, BHIP_WIN_AVG = 9, BHIP_WIN_COUNT = 10, BHIP_WIN_MIN = 11, BHIP_WIN_MAX = 12
} bhip_window_fn;
typedef enum {
    BHIP_FRAME_DEFAULT = 0, BHIP_FRAME_PARTITION = 1, BHIP_FRAME_ROWS_TO_CURRENT = 2, BHIP_FRAME_RANGE_TO_CURRENT = 3
} bhip_window_frame;
typedef struct {
    int32_t fn;              /* bhip_window_fn */
    bhip_expr arg;           /* ROW_NUMBER / RANK / DENSE_RANK: unused (nodes may be NULL) */
    int64_t offset;          /* LAG / LEAD: k, a plain number (not an expression) */
    int32_t frame;           /* bhip_window_frame */
    const char* name;        /* output field name */
} bhip_window_expr;
bhip_status bhip_plan_window(bhip_plan* input, int32_t n_partition, const bhip_expr* partition_by, int32_t n_order,
                             const bhip_sort_expr* order_by, int32_t n_fn, const bhip_window_expr* fns, bhip_plan** out);
/* a ROWS frame by signed offsets from the current row: -2 = 2 PRECEDING, 0 = CURRENT ROW, 3 = 3 FOLLOWING; start_unbounded = UNBOUNDED
 * PRECEDING, end_unbounded = UNBOUNDED FOLLOWING (the offset of an unbounded side is not read) */
typedef struct { int32_t start_unbounded, end_unbounded; int64_t start, end; } bhip_rows_frame;
/* bhip_plan_window with sliding frames: rows_frames is NULL (= bhip_plan_window) or n_fn pointers; a NULL entry leaves fns[i].frame as
 * it is, any other one is the frame of fns[i], whose `frame` must then be BHIP_FRAME_DEFAULT (BHIP_EINVAL otherwise). */
bhip_status bhip_plan_window_frames(bhip_plan* input, int32_t n_partition, const bhip_expr* partition_by, int32_t n_order,
                                    const bhip_sort_expr* order_by, int32_t n_fn, const bhip_window_expr* fns,
                                    const bhip_rows_frame* const* rows_frames, bhip_plan** out);
/* A frame in any units.  Each side is UNBOUNDED, CURRENT ROW or a signed OFFSET (-3 = 3 PRECEDING, +2 = 2 FOLLOWING: `i`, or `f` when
 * is_float).  The frame of row i is rows lo .. hi of its partition [ps, pe], or empty (no such row, or lo > hi):
 *   UNBOUNDED     ps / pe.
 *   CURRENT ROW   ROWS: row i; RANGE and GROUPS: i's first / last peer (any order keys, or none: the partition is one peer group).
 *   OFFSET        ROWS: bhip_rows_frame.  GROUPS: with the partition's peer groups numbered 0 .. G-1 and row i in group g, lo is the
 *                 first row of group max(g + start, 0) (none when g + start > G-1), hi the last row of group min(g + end, G-1) (none when
 *                 g + end < 0).  RANGE: exactly one order key, Int8..Int64, UInt8..UInt64, Float32, Float64, Date32, Date64 or Timestamp;
 *                 s = +1 ASC / -1 DESC.  Integer-typed keys (dates and timestamps in the column's unit) take Int64 offsets: row j
 *                 qualifies for the start when s (key_j - key_i) >= start and for the end when s (key_j - key_i) <= end, exactly, as in
 *                 unbounded integers.  Float keys take Float64 offsets (an Int64 one that a double holds exactly is converted):
 *                 t = key_i + s offset in Float64, row j qualifies when key_j >= t (start) / key_j <= t (end), mirrored for DESC, by IEEE
 *                 comparison (so -0.0 = +0.0 here, though they are not peers).  Only rows whose key is a number qualify (not NULL, not
 *                 NaN); a row i whose own key is NULL or NaN takes its peer bound.  lo = the first qualifying row, hi = the last.
 * Results are those of a ROWS frame over the same lo .. hi, the bit-reproducible float sums included; FIRST_VALUE / LAST_VALUE are
 * nullable like x, and always when start is an OFFSET > 0 or end an OFFSET < 0.  Floating SUM, AVG, MIN and MAX take at most 4096 rows
 * per frame: under RANGE / GROUPS the width is in the data, so a wider frame is BHIP_ENOTIMPL when the query runs; the same four from
 * an OFFSET or CURRENT ROW to UNBOUNDED FOLLOWING are BHIP_ENOTIMPL when the plan is made.  BHIP_EINVAL: unknown units or kind, a
 * start after the end (CURRENT ROW as 0), a NaN or infinite offset, and under RANGE with an OFFSET side anything but one order key of
 * the types above, a Float64 offset for an integer-typed key, an Int64 offset no double holds for a float key.  Any units UNBOUNDED
 * .. UNBOUNDED is PARTITION, RANGE / GROUPS UNBOUNDED .. CURRENT ROW is RANGE_TO_CURRENT, ROWS units are bhip_rows_frame. */
typedef enum { BHIP_FRAME_UNITS_ROWS = 0, BHIP_FRAME_UNITS_RANGE = 1, BHIP_FRAME_UNITS_GROUPS = 2 } bhip_frame_units;
typedef enum { BHIP_BOUND_UNBOUNDED = 0, BHIP_BOUND_CURRENT_ROW = 1, BHIP_BOUND_OFFSET = 2 } bhip_frame_bound_kind;
typedef struct { int32_t kind, is_float; int64_t i; double f; } bhip_frame_bound;
typedef struct { int32_t units, reserved; bhip_frame_bound start, end; } bhip_frame_spec;
/* bhip_plan_window_frames for frames in any units: specs is NULL (= bhip_plan_window) or n_fn pointers; a NULL entry leaves
 * fns[i].frame as it is, any other one is the frame of fns[i], whose `frame` must then be BHIP_FRAME_DEFAULT (BHIP_EINVAL otherwise). */
bhip_status bhip_plan_window_frame_specs(bhip_plan* input, int32_t n_partition, const bhip_expr* partition_by, int32_t n_order,
                                         const bhip_sort_expr* order_by, int32_t n_fn, const bhip_window_expr* fns,
                                         const bhip_frame_spec* const* specs, bhip_plan** out);
bhip_status bhip_plan_repartition(bhip_plan* input, int32_t scheme, int32_t n_exprs, const bhip_expr* hash_exprs,
                                  int32_t partition_count, bhip_plan** out);                         /* :133-164 */
bhip_status bhip_plan_coalesce_batches(bhip_plan* input, int64_t target_batch_size, bhip_plan** out);  /* :122-128 */
bhip_status bhip_plan_merge(bhip_plan* input, bhip_plan** out);                                       /* :129-132 */
bhip_status bhip_plan_global_limit(bhip_plan* input, int64_t limit, bhip_plan** out);                 /* :165-168 */
bhip_status bhip_plan_local_limit(bhip_plan* input, int64_t limit, bhip_plan** out);                  /* :169-172 */

/* ---- the wire plan ------------------------------------------------------------------------------
 * bhip_plan_from_proto: `impl TryInto<Arc<dyn ExecutionPlan>> for &protobuf::PhysicalPlanNode`
 * (rust/core/src/serde/physical_plan/from_proto.rs:58-346): `bytes` is the protobuf encoding of a PhysicalPlanNode
 * (rust/core/proto/ballista.proto:294-312) exactly as a task carries it (TaskDefinition.plan :531-534,
 * ExecutePartition.plan :451-458).  Expressions are planned against their input schema with DataFusion's coercion
 * rules (compile_expr, :348-364).  Every leaf (CsvScan / ParquetScan / ShuffleReader / UnresolvedShuffle) is offered
 * to `resolve` (may be NULL): it returns BHIP_OK with *out = a plan that produces the leaf's rows (a bhip_plan_memory, a
 * bhip_plan_arrow_stream over a CPU reader ...; ownership of that handle passes to the library), or BHIP_OK with *out = NULL to leave the leaf to the library:
 * a CsvScan over '|'-separated header-less local files becomes the device `.tbl` scan, a CsvScan over local files with
 * any other one-byte delimiter or a header the device CSV scan (both as bhip_plan_text_scan: files of any size, one batch per
 * slab; the node's batch_size is not used), any
 * other leaf an operator that describes itself and fails on execute with BHIP_EEXEC
 * (UnresolvedShuffleExec::execute, rust/core/src/execution_plans/unresolved_shuffle.rs:83-90).
 * `ctx` may be NULL when every leaf is left unresolved: the plan can then be inspected (bhip_plan_display, _schema,
 * _children) but not executed — what the CPU-only tests use. */
typedef enum {
    BHIP_LEAF_CSV_SCAN = 1, BHIP_LEAF_PARQUET_SCAN = 2, BHIP_LEAF_SHUFFLE_READER = 3, BHIP_LEAF_UNRESOLVED_SHUFFLE = 4
} bhip_leaf_kind;
typedef struct {                 /* PartitionLocation, ballista.proto:461-465 */
    const char* job_id;
    uint32_t stage_id, partition_id;
    const char* executor_id;
    const char* host;
    uint32_t port;
    int64_t num_rows, num_batches, num_bytes;       /* PartitionStats; -1 = not sent */
} bhip_partition_location;
typedef struct {
    int32_t kind;                                   /* bhip_leaf_kind */
    const char* path;                               /* CsvScan */
    int32_t n_filenames;
    const char* const* filenames;                   /* CsvScan partition files / ParquetScan files */
    int32_t has_projection, n_projection;
    const uint32_t* projection;                     /* indices into `fields` (CsvScan) / the file schema (ParquetScan) */
    int32_t n_fields;
    const bhip_column_desc* fields;                 /* CsvScan: the FILE's fields; shuffle leaves: the output schema */
    int32_t has_header;
    const char* delimiter;
    const char* file_extension;
    uint32_t batch_size, num_partitions;
    int32_t n_locations;
    const bhip_partition_location* locations;       /* ShuffleReader */
    int32_t n_stage_ids;
    const uint32_t* stage_ids;                      /* UnresolvedShuffle */
    uint32_t partition_count;
} bhip_leaf_desc;
typedef bhip_status (*bhip_leaf_resolver)(void* user, const bhip_leaf_desc* leaf, bhip_plan** out);
bhip_status bhip_plan_from_proto(bhip_ctx* ctx, const void* bytes, size_t len, bhip_leaf_resolver resolve, void* user,
                                 bhip_plan** out);
/* one LogicalExprNode (ballista.proto:14-45) rendered the way plan displays render expressions; for tools and tests */
bhip_status bhip_expr_from_proto_display(const void* bytes, size_t len, char* buf, size_t cap);

void bhip_plan_retain(bhip_plan* plan);
void bhip_plan_release(bhip_plan* plan);

/* ---- ExecutionPlan trait (query_stage.rs:49-85) ---------------------------------------------- */
/* as_any(): the operator's type name, e.g. "HashAggregateExec" */
const char* bhip_plan_name(const bhip_plan* plan);
/* schema(): fills up to `cap` entries, *n_cols = total number */
bhip_status bhip_plan_schema(const bhip_plan* plan, int32_t cap, const char** names, int32_t* dtypes,
                             int32_t* nullable, int32_t* n_cols);
/* output_partitioning() */
bhip_status bhip_plan_output_partitioning(const bhip_plan* plan, int32_t* scheme, int32_t* partition_count);
/* children(): NEW handles (the caller releases each) */
bhip_status bhip_plan_children(const bhip_plan* plan, int32_t cap, bhip_plan** children, int32_t* n_children);
/* with_new_children() */
bhip_status bhip_plan_with_new_children(const bhip_plan* plan, int32_t n, bhip_plan* const* children, bhip_plan** out);
/* async execute(partition) -> stream.  Blocking (wrap in spawn_blocking); re-entrant. */
bhip_status bhip_plan_execute(bhip_plan* plan, int32_t partition, bhip_stream** out);
/* Debug-style one-line-per-operator rendering (utils.rs:96-188 pretty printer) */
bhip_status bhip_plan_display(const bhip_plan* plan, char* buf, size_t cap);

/* ---- RecordBatchStream (memory_stream.rs:57-92) ------------------------------------------- */
/* stream.next(): *out = NULL at end of stream */
bhip_status bhip_stream_next(bhip_stream* stream, bhip_batch** out);
bhip_status bhip_stream_schema(const bhip_stream* stream, int32_t cap, const char** names, int32_t* dtypes,
                               int32_t* nullable, int32_t* n_cols);
void bhip_stream_release(bhip_stream* stream);
/* datafusion::physical_plan::collect(plan): executes every output partition in turn and returns all batches, in partition order
 * (the client-side `collect` of rust/core/src/execution_plans/... / SURVEY.md §8 a12).  At most `cap` batches are returned
 * (BHIP_EINVAL if the plan yields more); each one is released with bhip_batch_release. */
bhip_status bhip_plan_collect(bhip_plan* plan, int32_t cap, bhip_batch** out, int32_t* n_out);

/* hands the stream to an Arrow C Stream consumer (batches are copied to host as they are pulled);
 * the bhip_stream is consumed. */
bhip_status bhip_stream_export_arrow(bhip_stream* stream, struct ArrowArrayStream* out);
/* drains a stream like utils::write_stream_to_disk (rust/core/src/utils.rs:49-84) and reports
 * PartitionStats{num_rows,num_batches,num_bytes}; batches are handed to `sink` (may be NULL). */
typedef bhip_status (*bhip_batch_sink)(void* user, bhip_batch* batch);
bhip_status bhip_stream_drain(bhip_stream* stream, bhip_batch_sink sink, void* user, uint64_t* num_rows,
                              uint64_t* num_batches, uint64_t* num_bytes);

/* ---- Arrow IPC files: the two sides of a stage boundary ------------------------------------------------------
 * bhip_stream_write_ipc = utils::write_stream_to_disk (rust/core/src/utils.rs:49-84): drains the stream into an Arrow IPC
 * FILE at `path` (what the executor serves to the next stage, rust/executor/src/flight_service.rs:104-150) and reports
 * PartitionStats.  The stream is CONSUMED on every path, success or error (a NULL `stream` aside): the caller must NOT call
 * bhip_stream_release on it afterwards.
 * bhip_plan_ipc_files: a leaf over such files, one output partition per file — the local half of ShuffleReaderExec
 * (rust/core/src/execution_plans/shuffle_reader.rs:77-99).  Files written by arrow-rs / pyarrow are read as well
 * (metadata V4 or V5, no compression, no dictionaries; other files -> BHIP_ENOTIMPL).
 * bhip_ipc_write_file / bhip_ipc_open_file are the same on host-side Arrow C streams (no GPU involved). */
bhip_status bhip_stream_write_ipc(bhip_stream* stream, const char* path, uint64_t* num_rows, uint64_t* num_batches,
                                  uint64_t* num_bytes);
bhip_status bhip_plan_ipc_files(bhip_ctx* ctx, int32_t n_files, const char* const* paths, bhip_plan** out);
bhip_status bhip_ipc_write_file(struct ArrowArrayStream* stream, const char* path, uint64_t* num_rows, uint64_t* num_batches,
                                uint64_t* num_bytes);
bhip_status bhip_ipc_open_file(const char* path, struct ArrowArrayStream* out);

/* ---- hash repartition exchange support (RepartitionExec(Hash) across GPUs) -----------------
 * The per-row partition id is  bhip_row_hash(key columns) % n  (DESIGN.md "Row hash").  These
 * two calls split a device batch into n device batches (partition p = rows whose id is p, input
 * order kept) so the caller can exchange them (RCCL all-to-all) — used by the multi-GPU path. */
bhip_status bhip_batch_hash_partition(bhip_batch* batch, int32_t n_exprs, const bhip_expr* hash_exprs, int32_t n,
                                      bhip_batch** out /* n handles */);
/* concat: the rows of batches[0 .. n) in order, as one batch with the first batch's column names.  Every batch must have the first
 * one's column count and types (BHIP_EINVAL otherwise); a column of the result is nullable when it is in any of them.  n = 1 hands
 * the batch back as it is. */
bhip_status bhip_batch_concat(bhip_ctx* ctx, int32_t n, bhip_batch* const* batches, bhip_batch** out);

/* ---- exchange between the GPUs of one node (RCCL over xGMI, inside the library) -----------------------------
 * What a stage boundary is in the reference — partitions written as IPC files (rust/core/src/utils.rs:49-84) and pulled by
 * ShuffleReaderExec over Flight (rust/core/src/execution_plans/shuffle_reader.rs:77-99) — between processes that each
 * own one GPU of the node: batches move device to device.  One communicator per process and GPU; the 128-byte id made
 * by rank 0 (bhip_comm_unique_id) reaches the other ranks by whatever channel they share.  Collective calls: every rank
 * of the communicator must make the same call, with batches of ONE schema.  librccl is loaded at the first call. */
#define BHIP_COMM_ID_BYTES 128
typedef struct bhip_comm bhip_comm;
bhip_status bhip_comm_unique_id(uint8_t* id /* BHIP_COMM_ID_BYTES */);
bhip_status bhip_comm_create(bhip_ctx* ctx, const uint8_t* id, int32_t world, int32_t rank, bhip_comm** out);
/* Everything above the byte movers (block layout, header / count matrices, who sends what to whom, the streaming shuffle)
 * is one piece of code over a two-call transport; RCCL is one of three:
 * bhip_comm_create_loopback: `world` communicators inside ONE process on one device (any 128 bytes as the id; an id serves
 * one world once), each driven by its own thread; regions move with device-to-device copies after a host rendezvous.  It runs
 * the N-rank code paths on a single-GPU box (tests).
 * bhip_comm_create_host: the caller moves HOST bytes through two callbacks (0 = ok): an executor that only has its
 * Flight / TCP channel between processes, or a rehearsal over gloo.  Regions of one peer pair are matched in order. */
bhip_status bhip_comm_create_loopback(bhip_ctx* ctx, const uint8_t* id, int32_t world, int32_t rank, bhip_comm** out);
typedef struct bhip_comm_region { void* ptr; uint64_t bytes; int32_t peer; } bhip_comm_region;
typedef struct bhip_comm_host_transport {
    void* user;
    /* recv[r * bytes, (r + 1) * bytes) <- rank r's send[0, bytes) */
    int32_t (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes);
    /* one grouped exchange: every send reaches the matching receive of its peer */
    int32_t (*exchange)(void* user, int32_t n_sends, const bhip_comm_region* sends, int32_t n_recvs, const bhip_comm_region* recvs);
} bhip_comm_host_transport;
bhip_status bhip_comm_create_host(bhip_ctx* ctx, const bhip_comm_host_transport* transport, int32_t world, int32_t rank, bhip_comm** out);
void bhip_comm_release(bhip_comm* comm);
/* world, rank and the transport's name ("rccl" | "loopback" | "host"; valid while the communicator lives) */
bhip_status bhip_comm_info(bhip_comm* comm, int32_t* world, int32_t* rank, const char** transport);
/* wall seconds inside collective calls, bytes this rank sent to other ranks, calls — since the last reset */
bhip_status bhip_comm_stats(bhip_comm* comm, int32_t reset, double* seconds, uint64_t* bytes_out, uint64_t* calls);
/* the MergeExec side of a stage boundary: out[r] = rank r's batch, r = 0 .. world-1 (out[rank] is `mine`); the caller
 * releases every handle.  Small batches (partial aggregate states) travel in ONE ncclAllGather. */
bhip_status bhip_comm_all_gather(bhip_comm* comm, bhip_batch* mine, bhip_batch** out /* world handles */);
/* the shuffle of RepartitionExec(Hash(keys), world): parts[d] (bhip_batch_hash_partition) goes to rank d;
 * out[s] = what rank s held for this rank.  One grouped ncclSend / ncclRecv per peer pair. */
bhip_status bhip_comm_all_to_all(bhip_comm* comm, bhip_batch* const* parts /* world */, bhip_batch** out /* world handles */);
/* RepartitionExec(Hash([key_column], world)) (rust/core/src/serde/physical_plan/from_proto.rs:133-147) + the shuffle read
 * (rust/core/src/execution_plans/shuffle_reader.rs:77-99) in one collective call: *out = the rows of every rank's `batch`
 * whose key hashes to this rank, in source-rank order, input order within a source.  Fixed-width NULL-free columns with a
 * NULL-free integer key STREAM in chunks of `chunk_rows` rows (<= 0: 64 Mi): a count pass sizes the result exactly, a peer's
 * rows land at their final position, device memory beyond input and result is two chunks.  Anything else goes through
 * bhip_batch_hash_partition + bhip_comm_all_to_all + concat inside the call.  stats may be NULL. */
#define BHIP_SHUFFLE_MAX_PEERS 64
typedef struct bhip_shuffle_stats {
    uint64_t rows_in, rows_out, chunks, streamed;       /* streamed: 1 = the chunked path ran */
    uint64_t bytes_sent_remote, bytes_kept_local, staging_bytes;
    uint64_t rows_to[BHIP_SHUFFLE_MAX_PEERS];           /* rows of `batch` that went to each rank (the xGMI numerator) */
    double ms_count, ms_total;                          /* the count pass; the whole call (host wall clock) */
} bhip_shuffle_stats;
bhip_status bhip_comm_shuffle(bhip_comm* comm, bhip_batch* batch, const char* key_column, int64_t chunk_rows, bhip_batch** out,
                              bhip_shuffle_stats* stats);
/* The exchange as plan nodes, so that a rank's whole distributed query is ONE operator tree (one bhip_plan_collect per step).
 * AllGatherExec: executes every partition of `input`, all_gathers the result; `world` output partitions, partition r = rank
 * r's batch (what MergeExec over the previous stage's partitions reads, rust/scheduler/src/planner.rs:136-171).
 * ShuffleExchangeExec: executes every partition of `input`, bhip_comm_shuffle by `key_column`; one output partition.
 * The plan keeps the communicator alive.  Every rank must execute the same exchange nodes in the same order. */
bhip_status bhip_plan_all_gather(bhip_comm* comm, bhip_plan* input, bhip_plan** out);
bhip_status bhip_plan_shuffle(bhip_comm* comm, bhip_plan* input, const char* key_column, int64_t chunk_rows, bhip_plan** out);
/* The block form the exchange moves, for transports other than RCCL: header = 2 + 3 * columns int64 words (rows, block
 * bytes, then per column: data bytes, has offsets, has validity); the block holds every buffer, 64-byte aligned.
 * host_block NULL: only the header and *block_bytes are produced.  bhip_batch_unpack is the inverse (one copy to the
 * device; the columns are slices of it). */
bhip_status bhip_batch_pack(bhip_batch* batch, int64_t* header, int32_t header_cap, void* host_block, int64_t block_cap,
                            int64_t* block_bytes);
bhip_status bhip_batch_unpack(bhip_ctx* ctx, int32_t n_cols, const bhip_column_desc* schema, const int64_t* header,
                              const void* host_block, bhip_batch** out);

/* ---- synthetic TPC-H data (bench / tests) -------------------------------------------------- */
/* lineitem rows [row0,row0+n) at scale factor `sf` generated on the device; key64: Int64 order keys
 * (SF1000).  Columns: l_orderkey l_suppkey l_quantity l_extendedprice l_discount l_tax
 * l_returnflag l_linestatus l_shipdate [l_commitdate l_receiptdate when with_dates]. */
bhip_status bhip_tpch_lineitem(bhip_ctx* ctx, double sf, uint64_t seed, uint64_t row0, uint64_t n, int32_t key64,
                               int32_t with_dates, bhip_batch** out);
bhip_status bhip_tpch_orders(bhip_ctx* ctx, double sf, uint64_t seed, uint64_t row0, uint64_t n, int32_t key64,
                             bhip_batch** out);
/* The same with options.  sparse_keys: dbgen's order-key layout (the low 3 bits of the order number kept, the rest shifted up
 * by two: 8 of every 32 key values used — SF1000 keys reach 6 x 10^9 and need Int64); key_base is added to every order key
 * (small tables with keys beyond 2^32); columns: only these (NULL = all), in the table's column order. */
typedef struct bhip_tpch_opts {
    int32_t key64, with_dates, sparse_keys, n_columns;
    int64_t key_base;
    const char* const* columns;
} bhip_tpch_opts;
bhip_status bhip_tpch_lineitem_opts(bhip_ctx* ctx, double sf, uint64_t seed, uint64_t row0, uint64_t n, const bhip_tpch_opts* opts,
                                    bhip_batch** out);
bhip_status bhip_tpch_orders_opts(bhip_ctx* ctx, double sf, uint64_t seed, uint64_t row0, uint64_t n, const bhip_tpch_opts* opts,
                                  bhip_batch** out);

/* ---- measurement hooks --------------------------------------------------------------------- */
/* time (ms, HIP events on the stream the kernels ran on) and launch count of the dominant scan
 * kernel accumulated on this context since the last reset */
bhip_status bhip_ctx_kernel_time(bhip_ctx* ctx, int32_t reset, double* ms, uint64_t* launches);
/* every kernel timed since the last reset (BHIP_KERNEL_TIMING=1), one line per kernel: "name\tms\tlaunches\talgorithmic bytes\n" (bytes: 0 where the call site does not state them)
 * (NUL terminated; BHIP_EINVAL when `cap` is too small).  Waits for the timed launches to finish. */
bhip_status bhip_ctx_kernel_stats(bhip_ctx* ctx, int32_t reset, char* buf, size_t cap);
/* name of the kernel those launches ran ("" before the first timed launch); valid until the next call */
const char* bhip_ctx_kernel_name(bhip_ctx* ctx);
/* which instantiation of that kernel ran, where the call site says ("lean_generic", "lean_spec_q1", ...; "" otherwise);
 * valid until the next call */
const char* bhip_ctx_kernel_variant(bhip_ctx* ctx);
/* how the last wide-load scan + aggregate launch (timed or not) read its Utf8 group keys: "fixed" (every value of each key
 * column is known to have one width: no offsets are read), "offsets", or "none" (no Utf8 key); "" before the first such launch;
 * valid until the next call */
const char* bhip_ctx_lean_key_form(bhip_ctx* ctx);
/* which loaded column each chain step of that launch used, as a list of step numbers: "0,1,2,3,2" where the kernel formed step
 * 4's value from the column step 2 loaded (two steps of the plan read one column, and the kernel loaded it once); "none" where
 * every step loaded its own column; "" before the first such launch; valid until the next call */
const char* bhip_ctx_lean_step_alias(bhip_ctx* ctx);
/* how the last GlobalLimitExec / LocalLimitExec directly over a SortExec ran: "topk" (the rows that can be among the first k were
 * selected by a threshold on the first sort key, and only they were sorted), "topk_fallback" (the selection declined every batch —
 * too many candidates, a small batch, a first key it does not image — and the plain sort was cut to k), "sort" (the full-sort
 * route: the limit is not below the row count, or BHIP_NO_TOPK is set); "" before the first such execution; valid until the next call */
const char* bhip_ctx_sort_limit_form(bhip_ctx* ctx);
/* the table form of the HashJoinExec build side most recently built or probed on the context: "narrow" (one integer key or a pair
 * of 4-byte integer keys, unique build side), "packed" (the general table over 16-byte packed keys), "wide" (the table over row
 * hashes whose equality test reads the key columns: keys of any width; also reported when a probe batch whose keys outgrew the
 * packed key went through the wide table built beside a packed one); "" before the first build; valid until the next call */
const char* bhip_ctx_join_key_form(bhip_ctx* ctx);
/* how NestedLoopJoinExec ran the last probe batch on the context: "compare" (the filter is an AND of up to four column-to-column
 * comparisons: the fused kernel), "general" (any other filter: chunks of candidate pairs through the filter), "cross" (no filter:
 * the pairs are emitted directly), "exists" (SEMI / ANTI / RIGHT_SEMI / RIGHT_ANTI without a filter: nothing is enumerated);
 * "" before the first one; valid until the next call */
const char* bhip_ctx_nested_loop_form(bhip_ctx* ctx);
/* the probe kernel variant HashJoinExec's single-key path launched for its last probe batch: "rank/mapbuf" (the one-read kernel, the
 * packed map through a buffer descriptor), "rank/flat" (the same through flat loads and an explicit window test), "rank/bits" (the key-set
 * words alone: nothing staged, sorted one-column build side), each with "+perm" (unsorted build side), "+resid" (second key column),
 * "+rows8" (eight rows per lane) or "+gather" (no scalar map reads) where they apply; "filter/map" and "filter/table" (the general
 * kernel over the rank map / the CAS table, "+present" with the key-set bitmap in front of it, "+resid"); "" before the first one;
 * valid until the next call */
const char* bhip_ctx_join_probe_form(bhip_ctx* ctx);
/* compute units of the context's device (what the kernels size their grids by) */
int32_t bhip_ctx_device_cus(bhip_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* BALLISTA_HIP_H */
