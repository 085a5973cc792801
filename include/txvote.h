/*
 * txvote.h — C ABI of libtxvote.so, the MI355X-native TxVote admission path of go-txflow.
 *
 * This is the drop-in boundary: every entry point is what the reference's Go code would
 * bind through cgo for this path (the binding is shown in INTEGRATION.md).  Plain
 * pointers and sizes only; no HIP or torch types.  Caller buffers are read/written only
 * during the call (cgo pointer rules); the library copies into its own pinned host and
 * device buffers.  Return value: TXV_OK or a negative infrastructure error; per-vote
 * verdicts are never reported through the return value.
 *
 * Reference interfaces replaced (file:line in Fantom-foundation/go-txflow):
 *   txv_verify_batch   <- func (vote *TxVote) Verify(chainID string, pubKey crypto.PubKey) error
 *                         types/tx_vote.go:110-119  (ed25519 via tendermint VerifyBytes, :115)
 *   txv_verify_bytes   <- crypto.PubKey.VerifyBytes(msg, sig []byte) bool (tendermint
 *                         PubKeyEd25519, external; the call at types/tx_vote.go:115)
 *   txv_add_votes      <- func (txR *TxFlow) TryAddVote(vote *types.TxVote) (bool, error)
 *                         txflow/service.go:169-188 -> addVote :192-234
 *                         -> func (voteSet *TxVoteSet) AddVote(vote *TxVote) (bool, error)
 *                         types/vote_set.go:81-131, addVerifiedVote :143-166
 *   txv_query_tx       <- TxVoteSet.Stake / HasTwoThirdsMajority / HasTwoThirdsAny / HasAll
 *                         types/vote_set.go:178-227
 *   txv_get_votes      <- TxVoteSet.GetVotes / GetByAddress types/vote_set.go:57-64, 169-176
 *   txv_set_validators <- NewTxVoteSet(chainID, height, txHash, txKey, valSet)
 *                         types/vote_set.go:34-51 (state.ChainID / state.Validators, txflow/service.go:200-209)
 *   txv_signbytes      <- func (vote *TxVote) SignBytes(chainID string) []byte   types/tx_vote.go:83-89
 *   txv_txvote_size    <- func (vote *TxVote) Size() int                         types/tx_vote.go:144-150
 *   txv_keygen/txv_sign_votes <- MockPV.SignTxVote types/priv_validator.go:83-95 (load generator)
 *   txv_sig_keys       <- txVoteKey(tx) = sha256.Sum256(tx.Signature)   txvotepool/txvotepool.go:467-469
 *   txv_pool_*         <- TxVotePool (txvotepool/txvotepool.go): NewTxVotePool :56-75,
 *                         CheckTx/CheckTxWithInfo :180-261 (+ mapTxCache.Push :416-438, addTx :265-270),
 *                         Update :329-359, ReapMaxTxs :310-324, Flush :146-159, Size :136,
 *                         TxsBytes :141; removeTx :275-284
 *   txv_decode_msgs    <- Reactor.decodeMsg / cdc.UnmarshalBinaryBare(bz, &msg) into *TxVoteMessage
 *                         txvotepool/reactor.go:278-291 (codec: reactor.go:273-276, codec.go)
 *   txv_encode_msgs    <- cdc.MustMarshalBinaryBare(&TxVoteMessage{tx}) in broadcastTxRoutine
 *                         txvotepool/reactor.go:248 (the sending side of the same wire format)
 *   txv_gossip_msgs    <- the messages broadcastTxRoutine sends for a batch's admitted votes,
 *                         txvotepool/reactor.go:198-265, encoded on the device per batch
 *   txv_pool_receive   <- func (txR *Reactor) Receive(chID byte, src p2p.Peer, msgBytes []byte)
 *                         txvotepool/reactor.go:170-190 (decodeMsg + CheckTxWithInfo per message)
 *   txv_route_admitted / txv_submit_routed <- the Receive -> CheckTxWithInfo -> TryAddVote hand-off
 *                         (txvotepool/reactor.go:170-190 -> txvotepool.go:187-261 -> txflow/service.go:
 *                         123-166) across the GPUs of a node, CheckTx on one owner
 *   txv_sign_txs_submit / txv_sign_txs_wait <- Reactor.signTxRoutine's body for a batch of txs,
 *                         txvotepool/reactor.go:108-126: NewTxVote types/tx_vote.go:57-71 +
 *                         privVal.SignTxVote types/priv_validator.go:83-95, into a route buffer
 *   txv_pool_check_routed_submit / txv_submit_routed_checked <- the rest of signTxRoutine and what
 *                         follows it: txVotePool.CheckTx(txVote) txvotepool/reactor.go:126 ->
 *                         txvotepool.go:180-261, then checkMaj23Routine -> TryAddVote, from that
 *                         route buffer where it lies in HBM
 */
#ifndef TXVOTE_H
#define TXVOTE_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TXV_ABI_VERSION 2

/* ---- return codes (infrastructure) ---- */
#define TXV_OK 0
#define TXV_EINVAL (-22)
#define TXV_ENOMEM (-12)
#define TXV_EDEVICE (-5)      /* HIP error or no device */
#define TXV_ECAPACITY (-28)   /* configured capacity exceeded */
#define TXV_ESTATE (-1)       /* call order (e.g. no validator set) */

/* ---- per-vote status codes (status_out low 7 bits) ----
 * Mirror the (added, err) results of TxVoteSet.AddVote / TxVote.Verify:
 *   TXV_ADDED                 (true, nil)
 *   TXV_DUPLICATE             (false, nil)                            vote_set.go:110-111
 *   TXV_ERR_NIL               ErrVoteNil                              vote_set.go:93-95
 *   TXV_ERR_EMPTY_ADDR        ErrVoteInvalidValidatorAddress "Empty"  vote_set.go:97-99
 *   TXV_ERR_UNKNOWN_VALIDATOR ErrVoteInvalidValidatorIndex            vote_set.go:102-106
 *   TXV_ERR_NONDETERMINISTIC  ErrVoteNonDeterministicSignature        vote_set.go:112-113
 *   TXV_ERR_INVALID_SIGNATURE ErrVoteInvalidSignature                 tx_vote.go:115-117
 *   TXV_ERR_INVALID_VALIDATOR_ADDRESS ErrVoteInvalidValidatorAddress  tx_vote.go:111-113 (Verify only)
 *   TXV_ERR_SIGNBYTES         amino rejects the timestamp: the reference panics in SignBytes
 * Bit 7 (TXV_STATUS_FIRED) is set when the reference would run its commit side effects for
 * this vote: added && HasTwoThirdsMajority() (txflow/service.go:216), which re-fires on every
 * later added vote of a committed tx. */
#define TXV_ADDED 0
#define TXV_DUPLICATE 1
#define TXV_ERR_NIL 2
#define TXV_ERR_EMPTY_ADDR 3
#define TXV_ERR_UNKNOWN_VALIDATOR 4
#define TXV_ERR_NONDETERMINISTIC 5
#define TXV_ERR_INVALID_SIGNATURE 6
#define TXV_ERR_INVALID_VALIDATOR_ADDRESS 7
#define TXV_ERR_SIGNBYTES 8
#define TXV_STATUS_FIRED 0x80

typedef struct txv_ctx txv_ctx;

/* HBM footprint of a context (MI355X: 288 GB per GPU), all allocated up front:
 *   validator tables   n_vals x table size of the window (see TXV_CFG_WINDOW): 872 MB each at the
 *                      default radix-2^20 for <= 137 validators (87 GB for 100), within table_budget_mb
 *   base-point table   11.8 GB (radix-2^24; 43 GB at radix 2^26) per process and device, shared by
 *                      its contexts, plus 0.5 MB / 74 KB for the small windows
 *   TxFlow state       12 x max_txs x n_vals B of cells + 128 x max_accepted B of accepted votes +
 *                      64 x 2 (max_txs + max_batch) B of set table + key_arena_bytes (1M sets x 100
 *                      validators: 1.2 + 8.6 + 0.3 + 0.1 GB)
 *   per batch slot     ~420 B x max_batch of device columns, ~170 B x max_batch pinned host memory
 * txv_set_validators builds the validator tables on the device (K0: 0.9 s for 100 validators at
 * radix-2^20) for keys new to the context's table pool only; a set larger than the pool grows it
 * by an eighth more slots (within table_budget_mb). */
typedef struct {
  int32_t  device;          /* HIP device ordinal; -1 = current device */
  uint32_t max_batch;       /* votes per call (default 1<<20, at most 8<<20) */
  uint32_t max_txs;         /* TxVoteSets capacity (default 1<<20) */
  uint32_t max_validators;  /* default 1024 */
  uint32_t max_accepted;    /* accepted votes held (TxVoteSet.votes rows, one per ADDED vote, at most
                               one per (set, validator)); 0 = min(max_txs x n_vals, 2^26).  A batch that
                               would exceed it fails with TXV_ECAPACITY (reset with txv_reset_flow) */
  uint32_t max_msg_bytes;   /* unused since ABI 2 (SignBytes columns are sized per batch) */
  uint32_t flags;           /* TXV_CFG_* bits */
  uint32_t table_budget_mb; /* HBM budget for the per-validator fixed-base tables (default 114688 =
                               112 GiB): the default window is the largest of 20/18/16/14/12/10/8
                               whose tables fit (100 validators: radix-2^20, 87 GB) */
  uint64_t key_arena_bytes; /* device bytes for the TxHash strings of all TxVoteSets (each rounded up
                               to 8); 0 = 96 x max_txs + 1 MiB */
} txv_config;
/* verify with radix-16 tables (B staged in LDS, 74 KB/validator) instead of the wider
 * L2/HBM-resident tables */
#define TXV_CFG_TABLE_W4 0x1u
/* explicit fixed-base window in bits 8-15 (4, 8, 10, 12, 14, 16, 18, 20 or 21; 0 = auto: the
 * largest of 8..20 whose n_vals tables fit table_budget_mb, radix-2^20 for <= 137 validators): per
 * validator 74 KB / 0.5 MB / 1.7 MB / 5.8 MB / 20 MB / 67 MB / 252 MB / 872 MB / 1.70 GB (128-byte
 * entries).  Windows >= 12 run against the 11.8 GB radix-2^24 base-point table: 10 + ceil(256/W)
 * point additions per verified vote (32 / 29 / 26 / 25 / 23 at W = 12..20; the first B entry is
 * the starting point); W = 4 / 8 / 10: 2 * ceil(256/W) - 1 = 127 / 63 / 51.  W = 21 (on request
 * only; 12 positions over the 253 bits a scalar below L needs, the top one unsigned) runs against
 * the radix-2^26 base table: 9 + 12 = 21 additions (bench.py's C2 context) */
#define TXV_CFG_WINDOW(flags) (((flags) >> 8) & 0xFFu)
#define TXV_CFG_SET_WINDOW(w) (((uint32_t)(w) & 0xFFu) << 8)
/* votes per lane sharing one field inversion in the W >= 8 verify kernel, bits 16-19:
 * 2, 4 or 8 (8 needs the radix-2^24 or 2^26 base table), 1 = split (scalar-multiply kernel
 * stores R', a second kernel batch-inverts and encodes); 0 = auto: 8 when a launch's pending votes
 * fill >= 1.5 waves per SIMD (>= 768K) with a wide base table, else 1 (split) */
#define TXV_CFG_LANE_VOTES(flags) (((flags) >> 16) & 0xFu)
#define TXV_CFG_SET_LANE_VOTES(v) (((uint32_t)(v) & 0xFu) << 16)
/* base-point (B) table window, bits 20-27: 0 = auto (radix-2^24, 11.8 GB, over radix-2^12..2^20
 * validator tables; else the validator window; one table per process and device, shared by its
 * contexts; radix-2^26 by default under window 21); 24 over windows 12..20; 26 (43 GB, 10
 * additions for [s]B instead of 11) over windows 16..21; 20 / 22 over window 16 (0.9 / 3.2 GB,
 * 13 / 12 additions); or equal to the window */
#define TXV_CFG_B_WINDOW(flags) (((flags) >> 20) & 0xFFu)
#define TXV_CFG_SET_B_WINDOW(w) (((uint32_t)(w) & 0xFFu) << 20)

/* A batch of TxVotes (types/tx_vote.go:48-55) in structure-of-arrays form. */
typedef struct {
  uint32_t n;
  const uint8_t*  is_nil;      /* [n] or NULL: 1 = nil *TxVote */
  const int64_t*  height;      /* [n] Height */
  const uint8_t*  txhash;      /* TxHash string bytes, arena */
  const uint32_t* txhash_off;  /* [n] */
  const uint32_t* txhash_len;  /* [n] */
  const int64_t*  ts_sec;      /* [n] Timestamp: Unix seconds */
  const int32_t*  ts_nanos;    /* [n] Timestamp: nanoseconds [0, 1e9) */
  const uint8_t*  addr;        /* [n][20] ValidatorAddress bytes */
  const uint32_t* addr_len;    /* [n] len(ValidatorAddress) (0 = empty) */
  const uint8_t*  sig;         /* [n][64] Signature bytes (first 64) */
  const uint32_t* sig_len;     /* [n] len(Signature) */
  const uint8_t*  txkey;       /* [n][32] TxKey, or NULL (zero keys).  A new TxVoteSet takes its first
                                  vote's TxKey (txflow/service.go:201-207); accepted votes keep theirs
                                  (MakeCommit).  Not part of SignBytes (types/tx_vote.go:185-191) */
} txv_votes;

typedef struct {
  uint32_t vote_index;   /* index in the batch of the vote whose addition crossed 2/3 */
  uint32_t tx_index;     /* internal tx-set id */
  int64_t  sum;          /* stake of the set after the batch */
} txv_commit_event;

int  txv_init(const txv_config* cfg, txv_ctx** out);
void txv_destroy(txv_ctx* ctx);
const char* txv_last_error(txv_ctx* ctx);
int  txv_device_name(txv_ctx* ctx, char* buf, uint32_t cap);

/* Validator set + chain id.  pubs32: n x 32-byte ed25519 keys; powers: VotingPower, each in
 * [0, INT64_MAX / 8] with a total of at most INT64_MAX / 8 (tendermint's MaxTotalVotingPower: the
 * reference panics beyond it): TXV_EINVAL, with txv_last_error set, for a negative power or a larger
 * total, and the previous registry and its tally state stay as they were.  Within the range the
 * quorum Total*2/3 + 1 and every stake sum stay inside int64.  Power 0 is accepted.
 * Builds the per-validator tables on the device (K0) for the keys that have none: the context
 * keeps each key's tables in a slot of its table pool, so a set that re-orders, adds or drops
 * validators rebuilds only the new keys (and keys that left come back without a rebuild while
 * their slot was not reused).  Resets all tally state.  Replaces the validator set the
 * reference's TxFlow passes to each new VoteSet (txflow/service.go:200-207). */
int txv_set_validators(txv_ctx* ctx, const uint8_t* pubs32, const int64_t* powers, uint32_t n,
                       const char* chain_id, uint32_t chain_len);
/* addresses (n x 20, SHA-256(pub)[:20] computed on device) and decode flags of the set */
int txv_get_validator_info(txv_ctx* ctx, uint8_t* addr20_out, uint8_t* decode_ok_out, uint32_t cap);

/* TxVote.Verify(chainID, pubKey) for each vote.  pubs32: n x 32 caller-supplied keys, or NULL
 * to use the registry key whose address equals the vote's ValidatorAddress.  status_out:
 * TXV_ADDED (= nil error) / TXV_ERR_INVALID_VALIDATOR_ADDRESS / TXV_ERR_INVALID_SIGNATURE /
 * TXV_ERR_SIGNBYTES (and TXV_ERR_UNKNOWN_VALIDATOR when pubs32 == NULL and no key matches). */
int txv_verify_batch(txv_ctx* ctx, const txv_votes* votes, const uint8_t* pubs32, uint8_t* status_out);

/* crypto.PubKey.VerifyBytes(msg, sig) for n raw (pub, msg, sig) triples: tendermint
 * PubKeyEd25519.VerifyBytes (external, called at types/tx_vote.go:115) = len(sig) != 64 -> false,
 * else x/crypto ed25519.Verify(pub, msg, sig).  pubs32: n x 32 bytes; msgs: byte arena with
 * msg_off[i] / msg_len[i] (msg_len[i] <= TXV_MAX_RAW_MSG); sigs64: n x 64 bytes holding the first
 * 64 bytes of each signature, sig_len[i] its true length.  ok_out[i] = 1 accept, 0 reject. */
#define TXV_MAX_RAW_MSG 16384
int txv_verify_bytes(txv_ctx* ctx, const uint8_t* pubs32, const uint8_t* msgs, const uint32_t* msg_off,
                     const uint32_t* msg_len, const uint8_t* sigs64, const uint32_t* sig_len, uint32_t n,
                     uint8_t* ok_out);

/* TxFlow.TryAddVote for each vote in arrival order (votes[0] first).  Semantics are exactly
 * the sequential loop's; see SURVEY.md Appendix A.3.  ev_out (capacity ev_cap) receives one
 * event per tx whose 2/3 crossing happened in this batch, in arrival order of the crossing vote
 * (the order the reference runs its commit side effects); *n_ev their count.  Every decision is
 * made on the GPU: TxHash -> TxVoteSet routing (set ids in first-seen order), validator lookup,
 * pre-checks, SignBytes, verify, the first-accepted resolution per (set, validator), stake sums
 * and crossings; the host only moves the columns (registered memory: DMA only). */
int txv_add_votes(txv_ctx* ctx, const txv_votes* votes, uint8_t* status_out,
                  txv_commit_event* ev_out, uint32_t ev_cap, uint32_t* n_ev);

/* txv_add_votes split for pipelining (north_star: pinned SoA batches uploaded on a side stream):
 * txv_submit_votes copies the batch's columns into pinned memory (registered columns: none),
 * queues their upload on the copy stream and the kernel chain on the compute stream, and returns
 * a ticket without waiting; txv_wait_votes(ticket) waits for the results and reports exactly what
 * txv_add_votes would have.  At most four batches may be in flight (they share staged slots
 * 0-3 with txv_stage / txv_run_staged: do not mix the two on one context at the same time);
 * tickets are waited in submission order.  The staging of batch k+1 and its upload overlap the
 * kernels of batch k, and the staging of batch k+2 the upload of batch k+1.
 * Registered columns (txv_host_register) are read by DMA until txv_wait_votes returns for the
 * ticket; other caller buffers may be reused as soon as txv_submit_votes returns.  The TxVoteSet
 * readers (txv_query_tx*, txv_get_votes, txv_make_commit, ...) run after every submitted batch. */
int txv_submit_votes(txv_ctx* ctx, const txv_votes* votes, uint64_t* ticket);
int txv_wait_votes(txv_ctx* ctx, uint64_t ticket, uint8_t* status_out, txv_commit_event* ev_out, uint32_t ev_cap,
                   uint32_t* n_ev);

/* TxVoteSet.GetVotes / GetByAddress (types/vote_set.go:57-64, :169-176) for the set of txhash,
 * e.g. for the commit side effects (MakeCommit :242-259, TxVotePool.Update with GetVotes(),
 * txflow/service.go:222-226): the accepted vote of every validator that has one, in validator
 * index order (the reference iterates a Go map: unordered), as val_out[k] = validator index,
 * seq_out[k] = the vote's sequence number (count of votes passed to txv_add_votes /
 * txv_submit_votes / txv_run_staged since the last txv_reset_* before it + its index in its
 * batch), sig_out[k] = its 64 signature bytes.  *n_out = count (entries beyond cap are not
 * written).  Reflects every batch submitted so far. */
int txv_get_votes(txv_ctx* ctx, const uint8_t* txhash, uint32_t len, uint32_t* val_out, uint64_t* seq_out,
                  uint8_t* sig_out, uint32_t cap, uint32_t* n_out);

/* TxVotePool.Update's argument built on the device (txflow/service.go:216-227: after every fired
 * vote the commit path runs txV.Update(height, set.GetVotes())).  With the sink enabled, every
 * batch of the submit ring (txv_submit_votes, txv_submit_checked, txv_submit_routed, and
 * txv_add_votes through them) leaves, behind its tally, the list one Update per batch takes: the
 * sets that fired in the batch, ordered by the arrival index of their last fired vote, each set's
 * accepted votes so far -- as of the end of that batch -- in arrival order as one block.  That
 * list leaves the pool as the reference's Update after every fired vote does.  Per entry: the 64
 * signature bytes, TxVote.Size() and the set id (tx_index of the commit events).
 * txv_update_sink_enable: per-slot buffers of max_entries entries for the four-slot ring; 0
 *   disables and frees them (the default: no list is built).  Waits for the chains in flight;
 *   TXV_ESTATE while a submitted batch has not been waited for.
 * txv_update_list: the list of the batch `ticket` names, readable from the return of
 *   txv_wait_votes(ticket) until the slot's next batch is submitted (four submits later).  Any
 *   output may be NULL; *n_out = entries.  TXV_ESTATE when the sink is off, the ticket has not
 *   been waited for, its slot was reused, or the registry has more than 1024 validators (no list
 *   is built then); TXV_ECAPACITY when the batch's list exceeded max_entries (*n_out = the entries
 *   it needs; the batch's TxFlow results are not affected) or `cap` is below the list's length
 *   (*n_out = the length; nothing written). */
int txv_update_sink_enable(txv_ctx* ctx, uint32_t max_entries);
int txv_update_list(txv_ctx* ctx, uint64_t ticket, uint8_t* sig_out, uint32_t* size_out, uint32_t* set_out,
                    uint32_t cap, uint32_t* n_out);

/* TxStore.SaveTx's records built on the device (txflow/service.go:216-218: the commit block runs
 * txStore.SaveTx(set) for every fired vote; tx/store.go:83-117: db.Set("H:%X", TxVoteSet bytes) and
 * db.Set("C:%X", MakeCommit bytes)).  Both keys depend on the TxHash alone, so the last write wins:
 * every ADDED vote of a committed set fires, so a set's last fired vote of a batch is its last ADDED
 * vote of that batch, and the record written there is the one built from the set's accepted votes
 * as of the end of the batch.  With the sink enabled, every batch of the submit ring
 * (txv_submit_votes, txv_submit_checked, txv_submit_routed, and txv_add_votes through them) leaves,
 * behind its tally, one record per set that fired in it, ordered by the arrival index of each set's
 * last fired vote: writing them in that order leaves a key-value store as the reference's per-vote
 * cadence does.  (The height descriptor SaveTx also writes is the caller's state.LastBlockHeight.)
 * A record's bytes are those of txv_save_tx_bytes (CommitSigs in validator-index order), encoded
 * on the GPU; both sinks may be on at once.
 * txv_store_sink_enable: per-slot buffers of max_bytes bytes and max_records records for the
 *   four-slot ring; (0, 0) disables and frees them (the default: no record is built).  Waits for
 *   the chains in flight; TXV_ESTATE while a submitted batch has not been waited for.
 * txv_store_records: the records of the batch `ticket` names, readable from the return of
 *   txv_wait_votes(ticket) until the slot's next batch is submitted (four submits later; a submit
 *   into the slot while a read-out is copying fails with TXV_ESTATE).  out = the buffer as built:
 *   record k at off_out[k], a multiple of 16, its four parts -- "H:%X" key, TxVoteSet bytes, "C:%X"
 *   key, Commit bytes -- back to back with the lengths lens_out[4k .. 4k+3], zero padding up to the
 *   next record; set_out[k] = its set id (tx_index of the commit events).  Any output may be NULL;
 *   *n_out = records, *bytes_out = buffer bytes.  Only the bytes used are copied, on a stream of the
 *   read-out's own and without the context's lock, so batches in flight are not stalled.
 *   TXV_ESTATE when the sink is off, the ticket has not been waited for, its slot was reused, or the
 *   registry has more than 1024 validators (no record is built then); TXV_ECAPACITY when the batch
 *   overflowed the sink (*n_out, *bytes_out = what it needs; the batch's TxFlow results are not
 *   affected and the TxFlow is not poisoned) or `cap` / `rec_cap` is too small (*n_out, *bytes_out =
 *   the records' counts; nothing written). */
int txv_store_sink_enable(txv_ctx* ctx, uint64_t max_bytes, uint32_t max_records);
int txv_store_records(txv_ctx* ctx, uint64_t ticket, uint8_t* out, uint64_t cap, uint64_t* off_out,
                      uint32_t* lens_out, uint32_t* set_out, uint32_t rec_cap, uint32_t* n_out,
                      uint64_t* bytes_out);

/* The gossip sink: the sending side of CheckTx admission, built on the device.
 * broadcastTxRoutine (txvotepool/reactor.go:198-265) walks the pool list in order, sends
 * cdc.MustMarshalBinaryBare(&TxVoteMessage{Tx}) (:247-248) for every entry and skips the peer that
 * sent the vote itself (:245).  With the sink enabled, every batch of the submit ring
 * (txv_submit_votes, txv_submit_checked, txv_submit_routed, and txv_add_votes through them) leaves
 * one entry per non-nil vote, in arrival order, and the entries' TxVoteMessage bytes -- those of
 * txv_encode_msgs, amino-encoded on the GPU from the batch's columns in HBM -- in one buffer.  For
 * txv_submit_checked the non-nil votes are exactly those the pool admitted, and arrival order is
 * the order broadcastTxRoutine walks the pool list.  The chain runs on the flow stream before the
 * batch's tally, while that stream waits for the batch's verify; it touches no TxFlow state.  The
 * send itself stays the caller's, and so do the per-entry sender sets (txvotepool.go:213-250)
 * unless the pool keeps them (TXV_POOL_SENDERS: txv_pool_ticket_sent_by answers :245).  The
 * Update, store and gossip sinks may all be on at once.
 * Entry flags:
 *   TXV_GOSSIP_OK           the message is in the buffer
 *   TXV_GOSSIP_HOST         sig_len > 64 or addr_len > 20 (the columns hold only the first 64 / 20
 *                           bytes), or a message of 4 GiB or more: no bytes in the buffer (len 0);
 *                           the caller encodes this vote with txv_encode_msgs
 *   TXV_GOSSIP_UNENCODABLE  amino rejects the time: the reference's MustMarshalBinaryBare panics;
 *                           no bytes (len 0)
 * txv_gossip_sink_enable: per-slot buffers of max_bytes bytes and max_msgs entries for the
 *   four-slot ring; (0, 0) disables and frees them (the default: no kernel is enqueued).  Waits
 *   for the chains in flight; TXV_ESTATE while a submitted batch has not been waited for.  While
 *   the sink is on, batches are staged without the host validator lookup (the messages need the
 *   address bytes in HBM).
 * txv_gossip_msgs: the entries of the batch `ticket` names, readable from the return of
 *   txv_wait_votes(ticket) until the slot's next batch is submitted (four submits later; a submit
 *   into the slot while a read-out is copying fails with TXV_ESTATE, and so does a second read-out
 *   of the slot meanwhile).  out = the buffer as built: message k at off_out[k], a multiple of 16,
 *   len_out[k] bytes long, zero padding up to the next message; idx_out[k] = the vote's index in
 *   the batch (the caller skips the peers txv_pool_ticket_sent_by reports for vote idx, or, with
 *   a pool that keeps no Senders, the peer its own record names as the sender of vote idx);
 *   flag_out[k] as above.  Any output may be NULL; *n_out = entries, *bytes_out = buffer bytes.
 *   Only the bytes and descriptors used are copied, on a stream of the read-out's own and without
 *   the context's lock, so batches in flight are not stalled.
 *   TXV_ESTATE when the sink is off, the ticket has not been waited for, its slot was reused, or
 *   the batch was staged with txv_stage before the sink was enabled and took the host validator
 *   lookup (no messages are built for it: stage it again with the sink on);
 *   TXV_ECAPACITY when the batch overflowed the sink (*n_out, *bytes_out = what it needs; the
 *   batch's TxFlow results are not affected and the TxFlow is not poisoned) or `cap` / `msg_cap` is
 *   too small (*n_out, *bytes_out = the counts; nothing written).  No validator-count limit. */
#define TXV_GOSSIP_OK 0
#define TXV_GOSSIP_HOST 1
#define TXV_GOSSIP_UNENCODABLE 2
int txv_gossip_sink_enable(txv_ctx* ctx, uint64_t max_bytes, uint32_t max_msgs);
int txv_gossip_msgs(txv_ctx* ctx, uint64_t ticket, uint8_t* out, uint64_t cap, uint64_t* off_out,
                    uint32_t* len_out, uint32_t* idx_out, uint8_t* flag_out, uint32_t msg_cap,
                    uint32_t* n_out, uint64_t* bytes_out);

/* Tally readers for the TxVoteSet of txhash.  Returns 1 if the set exists, 0 if not. */
int txv_query_tx(txv_ctx* ctx, const uint8_t* txhash, uint32_t len, int64_t* sum, uint8_t* maj23);
/* the same for n TxHashes (txhash + off[i], len[i] bytes); any output may be NULL; txkey_out
 * [n][32] = TxVoteSet.TxKey (types/vote_set.go:24) */
int txv_query_txs(txv_ctx* ctx, const uint8_t* txhash, const uint32_t* off, const uint32_t* len, uint32_t n,
                  uint8_t* exists_out, int64_t* sum_out, uint8_t* maj23_out, uint8_t* txkey_out);

/* ---- commit side effects (txflow/service.go:216-232) ----
 * TxVoteSet.MakeCommit (types/vote_set.go:242-259): cdc.MustMarshalBinaryBare(Commit{TxHash,
 * Commits}) with one CommitSig (= the accepted TxVote, types/tx_vote.go:154-159) per validator that
 * has one, in validator-index order (the reference lists a Go map: any order; each CommitSig's
 * bytes are exact).  TXV_ESTATE without +2/3 (the reference panics) or without the set;
 * TXV_ECAPACITY (*len_out set) when cap is too small. */
int txv_make_commit(txv_ctx* ctx, const uint8_t* txhash, uint32_t len, uint8_t* out, uint64_t cap, uint64_t* len_out);
/* TxStore.SaveTx (tx/store.go:83-107): out = calcTxKey ("H:%X") | MustMarshalBinaryBare(TxVoteSet)
 * (TxHash, TxKey) | calcTxCommitKey ("C:%X") | MakeCommit bytes; lens_out = the four lengths. */
int txv_save_tx_bytes(txv_ctx* ctx, const uint8_t* txhash, uint32_t len, uint8_t* out, uint64_t cap,
                      uint64_t lens_out[4]);
uint32_t txv_num_tx_sets(txv_ctx* ctx);
int64_t  txv_total_power(txv_ctx* ctx);

/* amino encodings (host, no device work) */
int txv_signbytes(int64_t height, const uint8_t* txhash, uint32_t txhash_len, int64_t ts_sec,
                  int32_t ts_nanos, const char* chain_id, uint32_t chain_len, uint8_t* out, uint32_t cap);
int txv_txvote_size(int64_t height, uint32_t txhash_len, int64_t ts_sec, int32_t ts_nanos,
                    uint32_t addr_len, uint32_t sig_len);

/* ---- load generator (device signing, RFC 8032 deterministic) ---- */
/* seeds: n x 32 bytes -> pubs n x 32 bytes.  Keys are retained in ctx as signer slots. */
int txv_keygen(txv_ctx* ctx, const uint8_t* seeds32, uint32_t n, uint8_t* pubs_out);
/* Signs SignBytes(chain_id) of each vote with signer slot signer[i]; writes sig_out n x 64. */
int txv_sign_votes(txv_ctx* ctx, const txv_votes* votes, const uint32_t* signer, const char* chain_id,
                   uint32_t chain_len, uint8_t* sig_out);

/* ---- device-resident batches (benchmark / pipelined ingest) ----
 * Every AddVote batch (txv_add_votes, txv_submit_votes, txv_run_staged) runs on two device
 * streams: its verify chain (pre-checks, validator lookup, SignBytes, K1a/K1b) reads nothing the
 * TxFlow owns, so it starts as soon as its columns are uploaded, while the previous batch's
 * tally still runs; its TxFlow chain (TxHash keying, new set ids, tally) follows the previous
 * batch's on one stream, so results are those of the batches in submission order.
 * txv_stage: upload a batch's raw columns into device slot `slot` (0-3; TXV_ESTATE while the
 *   slot holds a txv_submit_votes batch: the submit ring uses slots 0 and 1).
 * txv_run_staged: enqueue the whole AddVote kernel chain on the staged batch and return (all
 *   four slots may be in flight: run 0, run 1, run 2, fetch 0, run 0, fetch 1, ...; a slot's
 *   next chain waits on the device for its previous one); results land in host memory for
 *   txv_fetch_staged.  kernel_ms_out (optional, 4 entries; makes the call
 *   wait): prep + SignBytes / verify (K1a + K1b) / tally after verify / total device time of
 *   this run, measured with HIP events on the streams the kernels run on.
 * txv_slot_kernel_ms: the same 4 times for the slot's last run, waiting for it if needed.
 * txv_slot_verify_ms: the verify time of the slot's last run split in two (2 entries): K1a
 *   (challenge, SHA-512 mod L) and K1b (the double scalar multiply, encode and compare).
 *   Measurement only, no reference counterpart. */
int txv_stage(txv_ctx* ctx, uint32_t slot, const txv_votes* votes);
int txv_run_staged(txv_ctx* ctx, uint32_t slot, float* kernel_ms_out);
int txv_fetch_staged(txv_ctx* ctx, uint32_t slot, uint8_t* status_out, txv_commit_event* ev_out,
                     uint32_t ev_cap, uint32_t* n_ev);
int txv_slot_kernel_ms(txv_ctx* ctx, uint32_t slot, float* kernel_ms_out);
int txv_slot_verify_ms(txv_ctx* ctx, uint32_t slot, float* k1a_k1b_ms_out);
/* caller host memory the AddVote path may DMA from directly (hipHostRegister): columns of a
 * txv_votes batch lying inside a registered range skip the staging copy */
int txv_host_register(txv_ctx* ctx, void* ptr, uint64_t bytes);
int txv_host_unregister(txv_ctx* ctx, void* ptr);
/* ---- multi-GPU: votes shard by SHA-256(TxHash)[0] mod n_shards; each shard's
 * commit state is packed as [n_sets u32][1 u32][bitmap: ceil(cap/32) u32][sums: cap i64]
 * [digests: cap x 16 B], set ids in the shard's first-seen order.  digest = SHA-256(TxHash
 * bytes)[0:16] (whose byte 0 mod n_shards is the shard): every rank can name every other rank's
 * TxVoteSets -- their commit bits and stakes -- from the gathered buffers alone ---- */
int txv_shard_of(const uint8_t* txhash, const uint32_t* off, const uint32_t* len, uint32_t n, uint32_t n_shards,
                 uint32_t* shard_out);
uint64_t txv_commit_state_bytes(uint32_t n_sets_cap);
/* this context's state into caller device memory (e.g. an RCCL all-gather buffer) */
int txv_pack_commit_state(txv_ctx* ctx, void* dst_dev, uint32_t n_sets_cap);
/* the same packed state written by the device at the end of every batch that runs in slot
 * `slot` (0-3: staged slot, or the txv_submit_votes ticket t with (t - 1) % 2 == slot), in
 * stream order before the batch's results are reported: once txv_fetch_staged / txv_wait_votes
 * returns for the batch, dst_dev holds the state as of that batch, even when the next batch is
 * already running.  dst_dev = NULL removes the sink.  For an all-gather per batch with two
 * batches in flight (txvote's per-shard commit exchange). */
int txv_set_commit_sink(txv_ctx* ctx, uint32_t slot, void* dst_dev, uint32_t n_sets_cap);
/* the context's flow stream (hipStream_t): every batch's TxFlow chain (keying, tally, commit
 * sink pack) runs on it in submission order.  A collective enqueued on it right after
 * txv_run_staged / txv_submit_votes (e.g. the per-batch RCCL all-gather of the commit sink)
 * reads the sink after that batch's pack and the next batch's TxFlow chain queues behind it, so
 * no host thread has to wait for the exchange.  Valid until txv_destroy. */
void* txv_flow_stream(txv_ctx* ctx);
/* the same packed by the device, copied into caller host memory (host-side gathers) */
int txv_read_commit_state(txv_ctx* ctx, void* dst_host, uint32_t n_sets_cap);
/* host-side pack (from per-set committed flags and sums) and unpack of the same layout */
int txv_commit_state_pack_host(uint32_t n_sets, const uint8_t* committed, const int64_t* sums, const uint8_t* digests,
                               uint32_t n_sets_cap, void* dst);
int txv_commit_state_unpack(const void* src, uint32_t n_sets_cap, uint32_t* n_sets, uint8_t* committed, int64_t* sums,
                            uint8_t* digests, uint32_t cap);
/* ---- multi-GPU ingest route (replaces the reactor -> TxFlow hand-off of
 * txvotepool/reactor.go:170-190 -> txvotepool.go:187-261 -> txflow/service.go:123-166 across
 * ranks).  TxVotePool is one order-dependent LRU with one Size cap, so CheckTx runs once for the
 * node, on its owner (reactor) rank; each vote it admits belongs to the rank txv_shard_of names.
 * txv_route_admitted packs, on the owner's GPU, every admitted vote (pool_status[i] ==
 * TXV_POOL_OK; pool_status NULL = all) into the buffer of its rank r at dst_dev + r * stride, in
 * arrival order, and returns each rank's txv_route_meta (the header's values: the receiving rank
 * needs n, max_txhash_len and the byte count before it receives); synchronous (dst_dev is written
 * when it returns).
 * Sizes: dst_dev and stride are multiples of 16 (the kernels store 16 bytes at a time at dst_dev +
 * r * stride + a column offset; TXV_EINVAL otherwise, from every route call), and stride >=
 * txv_route_bytes(votes->n, TxHash arena extent, flags) (TXV_EINVAL below that).  A rank's buffer
 * holds the sum of its votes' TxHash lengths, which exceeds the extent when votes share TxHash
 * offsets: a rank whose buffer would not fit its stride is refused -- nothing is written into its
 * region, its meta carries the true n, arena_bytes and bytes (the size it needs) with reserved = 1,
 * and the call returns TXV_ECAPACITY; the other ranks' buffers are complete and valid.  A stride
 * of txv_route_bytes(n, max(extent, sum of the non-nil votes' TxHash lengths), flags) fits every
 * split.  The
 * node's collective then sends buffer r to rank r as it is (RCCL over xGMI: no host copy), and
 * rank r runs its TxFlow chain straight from it: txv_submit_routed (a txv_submit_votes ticket,
 * collected by txv_wait_votes; the buffer may be reused once the call returns).  Buffer layout
 * (go-txflow_amd/csrc/route.h): a 64-byte header, then the txv_votes columns at 16-byte aligned
 * offsets, TxHash offsets relative to the buffer's own arena; a nil vote (TXV_ROUTE_NIL) carries
 * an empty TxHash and goes to the shard of "".  txv_route_view: a txv_votes view of a buffer
 * copied to host memory (pointers into buf).  txv_route_pack_host: the same buffers built on the
 * host (no GPU; the parity reference of the device route and the CPU test path). */
#define TXV_ROUTE_TXKEY 0x1u   /* the buffers carry the TxKey column */
#define TXV_ROUTE_NIL 0x2u     /* the buffers carry the is_nil column */
typedef struct {
  uint32_t n;                /* votes routed to the rank */
  uint32_t max_txhash_len;   /* their longest TxHash (the receiver's SignBytes bound) */
  uint32_t flags;            /* TXV_ROUTE_* */
  uint32_t reserved;         /* 1: the rank was refused (bytes > stride), its region untouched */
  uint64_t arena_bytes;      /* TxHash bytes */
  uint64_t bytes;            /* the buffer's size (txv_route_bytes) */
} txv_route_meta;
uint64_t txv_route_bytes(uint32_t n, uint64_t arena_bytes, uint32_t flags);
int txv_route_admitted(txv_ctx* ctx, const txv_votes* votes, const uint8_t* pool_status, uint32_t n_shards,
                       void* dst_dev, uint64_t stride, txv_route_meta* meta_out);
/* txv_route_admitted for the batch pool_ticket (txv_pool_check_submit on the same batch, the
 * pool's cache in HBM) is deciding: while the batch is in the pool engine's flight slot the route
 * kernels read its statuses and the signatures the CheckTx uploaded in HBM, behind the decisions
 * (no host round trip, the signatures not uploaded again); otherwise the ticket's statuses are
 * taken on the host.  The same buffers and metas as txv_route_admitted with those statuses; the
 * pool ticket is still the caller's to wait.  Takes the route lock, the pool's, the context's. */
int txv_route_checked(txv_ctx* ctx, const txv_votes* votes, struct txv_pool* pool, uint64_t pool_ticket, uint32_t n_shards,
                      void* dst_dev, uint64_t stride, txv_route_meta* meta_out);
/* The route as a submit / wait pair (the hop reactor.go:170-190 -> txvotepool.go:187-261 ->
 * service.go:123-166 pipelined like its neighbours txv_pool_check_submit / txv_submit_checked):
 * up to TXV_ROUTE_RING routes in flight per context, ticket t on ring entry (t - 1) %
 * TXV_ROUTE_RING, each entry with its own staging buffers and scratch.  A submit whose entry
 * still holds an unwaited ticket returns TXV_ESTATE and changes nothing; waits may come in any
 * order.  The route kernels of consecutive tickets run in submission order; the route lock is held
 * for the submit only, never across a wait.
 * txv_route_submit_admitted: txv_route_admitted's first half (the columns and pool_status staged
 * and uploaded, the kernels enqueued); returns without waiting for the GPU.
 * txv_route_submit_checked: txv_route_checked's first half.  While the CheckTx batch is in the
 * pool engine's flight slot the call waits for nothing on the GPU: the columns go through the
 * entry's pinned buffers on the copy stream, the statuses and signatures come from the flight
 * slot on the key stream behind the decisions, the kernels run behind them.  Only a pool ticket no
 * longer in the engine can block: its statuses are taken on the host, which may finish earlier
 * pool tickets first.
 * txv_route_wait: waits for the ticket's kernels with no lock held, copies its n_shards metas to
 * meta_out and frees the entry; dst_dev is written when it returns.  TXV_ECAPACITY: a rank was
 * refused (meta.reserved = 1; see Sizes above), the other ranks' buffers are valid.  TXV_EDEVICE:
 * the pool engine's look-back error word was set behind the decisions the route read (the
 * statuses are not trusted: ship nothing).  TXV_ESTATE: no such ticket in flight.
 * The caller keeps the destination regions of in-flight tickets apart.  Host columns may be reused
 * once the submit returns; memory registered with txv_host_register is read until the wait (the
 * rule of txv_pool_check_submit).  txv_route_admitted / txv_route_checked are submit + wait on the
 * same code (TXV_ESTATE too when four tickets are unwaited); one that leaves the ring idle skips
 * to the next ticket of its own entry, so a caller that never pipelines uses one entry.  txv_sync, txv_reset_flow and txv_destroy wait for the routes in flight first. */
#define TXV_ROUTE_RING 4
int txv_route_submit_admitted(txv_ctx* ctx, const txv_votes* votes, const uint8_t* pool_status, uint32_t n_shards,
                              void* dst_dev, uint64_t stride, uint64_t* route_ticket);
int txv_route_submit_checked(txv_ctx* ctx, const txv_votes* votes, struct txv_pool* pool, uint64_t pool_ticket,
                             uint32_t n_shards, void* dst_dev, uint64_t stride, uint64_t* route_ticket);
int txv_route_wait(txv_ctx* ctx, uint64_t route_ticket, txv_route_meta* meta_out);
int txv_route_pack_host(const txv_votes* votes, const uint8_t* pool_status, uint32_t n_shards, void* dst,
                        uint64_t stride, txv_route_meta* meta_out);
int txv_route_view(const void* buf, uint64_t bytes, txv_votes* out);
int txv_submit_routed(txv_ctx* ctx, const void* buf_dev, const txv_route_meta* meta, uint64_t* ticket);

/* ---- sign by batch on the device: a validator's own TxVotes built in HBM ----
 * <- Reactor.signTxRoutine's body (txvotepool/reactor.go:108-126) for a batch of mempool txs:
 * NewTxVote(LastBlockHeight, TxHash(tx), TxKey(tx), addr) (types/tx_vote.go:38-45,57-71), then
 * privVal.SignTxVote(chainID, &vote) (types/priv_validator.go:83-95).  The votes are built and
 * signed on the GPU and written as ONE route buffer (the layout of txv_route_admitted, flags
 * TXV_ROUTE_TXKEY, no nil column) at dst_dev: what txv_submit_routed runs TxFlow from, txv_route_view
 * reads on the host after a copy, and the multi-GPU path ships as it is.
 *
 * signer: a txv_keygen slot.  Chain id: the one txv_set_validators gave the context.  height:
 * state.LastBlockHeight.  Vote i (tx order) carries Height = height, TxKey = SHA-256(tx_i), TxHash =
 * the 64 upper-case hex characters of that digest (at offset 64 i of the buffer's arena), the
 * caller's timestamp (the time.Now() NewTxVote stamps), ValidatorAddress = SHA-256(pub)[:20] of the
 * signer, Signature = RFC 8032 Ed25519 over SignBytes(chainID): the bytes x/crypto's deterministic
 * ed25519.Sign and txv_sign_votes produce.  *meta_out = the buffer's meta (n, max_txhash_len 64,
 * flags, arena_bytes 64 n, bytes).  Every byte of [dst_dev, dst_dev + meta.bytes) is written,
 * whatever the memory held: the buffer is byte-equal to txv_route_pack_host of the same votes.
 *
 * "Only sign if I'm a validator" (reactor.go:111): when the signer's public key is not in the
 * context's registry the call succeeds with a buffer of zero votes (meta.n = 0).
 *
 * TXV_ESTATE without a validator set, or when the ring entry holds an unwaited ticket: up to
 * TXV_SIGN_RING signs in flight, ticket t on entry (t - 1) % TXV_SIGN_RING, waits in any order.
 * TXV_EINVAL when signer is not a slot, n > max_batch or n >= 2^26 (the buffer's TxHash offsets,
 * 64 i, are 32-bit), cap < txv_sign_txs_bytes(n), dst_dev is not
 * 16-byte aligned, or a timestamp is outside amino's time range (ts_nanos outside [0, 1e9), seconds
 * outside years 1..9999: the rule txv_signbytes applies).  The reference swallows a SignTxVote error
 * and runs CheckTx on the unsigned vote (reactor.go:120-122), and its time.Now() never leaves that
 * range; a vote this library cannot encode is refused instead.  A refused call writes nothing.
 *
 * The submit enqueues everything and returns without waiting for the GPU.  Host tx bytes and
 * timestamps may be reused once it returns.  txv_sign_txs is submit + wait on the same code.
 * txv_sync, txv_reset_flow, txv_keygen, txv_set_validators and txv_destroy wait for the signs in
 * flight first.  A txv_set_validators or txv_keygen that another thread runs while a submit is
 * copying its txs makes that submit fail with TXV_ESTATE (nothing enqueued or written).  A
 * synchronous call that leaves the ring idle takes the same ring entry again next time (its
 * tickets then advance by TXV_SIGN_RING), so a caller that never pipelines uses one entry's staging.
 *
 * Custody: the keys live in the context as txv_keygen left them (expanded secret scalar and nonce
 * prefix in device memory).  The table lines the walk reads and the variable-time field inversion
 * depend on the nonce: this is MockPV-grade signing (types/priv_validator.go:83-95), NOT
 * constant-time, and not a replacement for privval custody of a production key. */
typedef struct {
  uint32_t n;
  const uint8_t*  tx;        /* raw tx bytes, arena */
  const uint64_t* tx_off;    /* [n] */
  const uint32_t* tx_len;    /* [n]; 0 is a valid tx */
  const int64_t*  ts_sec;    /* [n] the Timestamp NewTxVote stamps (time.Now(), tx_vote.go:57-71): the caller's */
  const int32_t*  ts_nanos;  /* [n] */
} txv_txs;
#define TXV_SIGN_RING 2
/* = txv_route_bytes(n, 64 * n, TXV_ROUTE_TXKEY) */
uint64_t txv_sign_txs_bytes(uint32_t n);
int txv_sign_txs_submit(txv_ctx* ctx, const txv_txs* txs, uint32_t signer, int64_t height, void* dst_dev,
                        uint64_t cap, uint64_t* sign_ticket);
int txv_sign_txs_wait(txv_ctx* ctx, uint64_t sign_ticket, txv_route_meta* meta_out);
int txv_sign_txs(txv_ctx* ctx, const txv_txs* txs, uint32_t signer, int64_t height, void* dst_dev, uint64_t cap,
                 txv_route_meta* meta_out);
/* measurement: device time (ms) of the last waited sign chain, by events on the stream it ran on */
int txv_sign_txs_ms(txv_ctx* ctx, float* ms);
/* the meta txv_sign_txs_wait will return for n txs and this signer (n = 0 for a signer outside the
 * registry: "only sign if I'm a validator", txvotepool/reactor.go:111), so that
 * txv_pool_check_routed_submit and txv_submit_routed_checked can be enqueued behind an unwaited
 * txv_sign_txs_submit.  TXV_ESTATE without a validator set, TXV_EINVAL when signer is not a slot or
 * n > max_batch. */
int txv_sign_txs_meta(txv_ctx* ctx, uint32_t n, uint32_t signer, txv_route_meta* meta_out);
/* measurement / self-test only, like txv_fe_selftest: enc_out[i] = canonical encoding of
 * [scalars32[i]]B through the signer's walk and encode kernels (scalars little-endian, any 256-bit
 * value below 2^253; TXV_EINVAL above, TXV_ESTATE without a validator set) */
int txv_scalarmult_base(txv_ctx* ctx, const uint8_t* scalars32, uint32_t n, uint8_t* enc_out);

/* ---- LoadTxCommit by batch on the device: stored Commits back into TxFlow ----
 * <- TxStore.LoadTxCommit (tx/store.go:67-80), reached from TxFlow.LoadCommit
 * (txflow/service.go:115-120), for a batch of stored Commit records: the bytes
 * cdc.MustMarshalBinaryBare(set.MakeCommit()) that SaveTx wrote under "C:%X" (tx/store.go:83-107) --
 * what txv_make_commit, txv_save_tx_bytes and the store sink produce -- decoded on the GPU into ONE
 * route buffer at dst_dev (the layout of txv_route_admitted, flags TXV_ROUTE_TXKEY | TXV_ROUTE_NIL).
 * Record k's CommitSigs are the consecutive votes first_vote[k] .. first_vote[k + 1] - 1, in the
 * order the record lists them.  txv_submit_routed on that buffer re-verifies every signature and
 * re-tallies every set: the restore of committed sets after txv_reset_flow or a restart, and the
 * check of a Commit received from elsewhere.  The load itself reads and writes no TxFlow state and
 * needs no validator set.  The database read stays the caller's, as the write does.
 *
 * The decode rules are csrc/load_dev.h's header (amino as restated in oracle/wire.c; PARITY UNPINNED
 * beyond the records this library and the oracle write).  Per record, rec_status:
 *   TXV_COMMIT_OK       decoded; TXV_COMMIT_CORRUPT  an amino error in the envelope or in any
 *   element (LoadTxCommit panics): the record gives no votes; TXV_COMMIT_EMPTY  length 0 (db.Get
 *   found nothing, LoadTxCommit returns nil): no votes.
 * A zero-length element is a nil *CommitSig: is_nil = 1, every other column zero.  A vote carries its
 * CommitSig's own TxHash, not the enclosing Commit's (the reference compares neither with the
 * other).  sig_len > 64 and addr_len > 20 keep their true lengths with the first 64 / 20 bytes.
 *
 * recs: host memory; record k is the len[k] bytes at recs + off[k], at any alignment (off[k] +
 * len[k] <= recs_bytes; recs_bytes < 2^32, as for txv_decode_msgs).  A txv_store_records read-out can
 * be passed as it is: record k's Commit part is at off_out[k] + lens[4k] + lens[4k+1] + lens[4k+2],
 * lens[4k+3] bytes long.  The bytes are uploaded through the ring entry's pinned staging and may be
 * reused once the submit returns; from registered memory (txv_host_register) they are uploaded
 * directly and must stay unchanged until the wait.
 *
 * txv_load_commits_bytes(max_votes, commit_bytes) = txv_route_bytes(max_votes, commit_bytes,
 * TXV_ROUTE_TXKEY | TXV_ROUTE_NIL); with commit_bytes = the sum of the len[k] it bounds the arena of
 * any input these encoders wrote (every TxHash byte of the arena is a byte of some record).  dst_dev and cap must be
 * multiples of 16 (TXV_EINVAL otherwise, as from the route calls).  The buffer's size is decided on
 * the device: when it exceeds cap nothing is written to dst_dev at all, the wait returns
 * TXV_ECAPACITY, and *meta_out carries the true n, arena_bytes and bytes with reserved = 1
 * (txv_route_admitted's convention); rec_status and first_vote are valid all the same.
 *
 * A ring of TXV_LOAD_RING loads in flight, ticket t on entry (t - 1) % TXV_LOAD_RING, waits in any
 * order; a submit into an entry that holds an unwaited ticket returns TXV_ESTATE and changes
 * nothing, as does a wait for a ticket not in flight.  txv_sync, txv_reset_flow and txv_destroy wait
 * for the loads in flight first.  The chain runs on the context's copy and key streams.
 * Outputs of the wait (each may be NULL): meta_out; rec_status [n_records]; first_vote
 * [n_records + 1]; rec_txhash_off / rec_txhash_len [n_records]: Commit.TxHash as an offset into recs
 * and a length (0 when the field is absent or the record is not OK).  The wait takes n_records from
 * the submit.  txv_load_commits is submit + wait. */
#define TXV_COMMIT_OK 0
#define TXV_COMMIT_CORRUPT 1
#define TXV_COMMIT_EMPTY 2
#define TXV_LOAD_RING 2
uint64_t txv_load_commits_bytes(uint32_t max_votes, uint64_t commit_bytes);
int txv_load_commits_submit(txv_ctx* ctx, const uint8_t* recs, uint64_t recs_bytes, const uint64_t* off,
                            const uint32_t* len, uint32_t n_records, void* dst_dev, uint64_t cap,
                            uint64_t* load_ticket);
int txv_load_commits_wait(txv_ctx* ctx, uint64_t load_ticket, txv_route_meta* meta_out, uint8_t* rec_status,
                          uint32_t* first_vote, uint64_t* rec_txhash_off, uint32_t* rec_txhash_len);
int txv_load_commits(txv_ctx* ctx, const uint8_t* recs, uint64_t recs_bytes, const uint64_t* off, const uint32_t* len,
                     uint32_t n_records, void* dst_dev, uint64_t cap, txv_route_meta* meta_out, uint8_t* rec_status,
                     uint32_t* first_vote, uint64_t* rec_txhash_off, uint32_t* rec_txhash_len);
/* measurement: device time (ms) of the last waited load's kernels, like txv_sign_txs_ms */
int txv_load_commits_ms(txv_ctx* ctx, float* ms);

/* device pointer + byte size of the per-set committed bitmap (1 bit per tx-set id) */
int txv_commit_bitmap(txv_ctx* ctx, void** dev_ptr, uint64_t* bytes);
/* device-to-device copy of the commit bitmap into caller device memory (e.g. an RCCL buffer) */
int txv_copy_commit_bitmap(txv_ctx* ctx, void* dst_dev, uint64_t bytes);
/* device-to-device copy of the per-set stake sums (int64, set ids 0..n_sets-1) into caller device
 * memory: with the commit bitmap, the per-shard state a multi-GPU run all-gathers */
int txv_copy_set_sums(txv_ctx* ctx, void* dst_dev, uint32_t n_sets);
/* measured integer-VALU issue rates of this device (lane-ops/s): v_add_u32 and v_mad_u64_u32 */
int txv_valu_probe(txv_ctx* ctx, double* add_lane_ops_per_s, double* mad_lane_ops_per_s);
/* fixed-base window of the current validator tables (4..20), 0 before txv_set_validators */
int txv_table_window(txv_ctx* ctx);
/* keys whose tables the last txv_set_validators built (the others were already in the pool) */
int txv_validator_tables_built(txv_ctx* ctx);
/* host bytes the last staged batch (txv_stage / txv_submit_votes / txv_add_votes) sent over
 * PCIe: columns whose every element is equal are filled on the device instead, and the TxKey
 * column is decoded on the device from TxHash when every non-nil vote's TxKey is the 32 bytes its
 * 64-character upper-hex TxHash spells (TxKey = SHA-256(tx), TxHash = its %X, types/tx_vote.go:38-45) */
int64_t txv_staged_bytes(txv_ctx* ctx);
/* window of the base-point table the verify kernel uses (>= the validator window) */
int txv_base_window(txv_ctx* ctx);
/* empty every TxVoteSet (votes, stake, commit flags) keeping the validator set; tx-set ids
 * already assigned stay assigned (their sets read as empty).  Both resets run in stream order
 * after every batch already submitted; vote sequence numbers restart at 0 */
int txv_reset_tally(txv_ctx* ctx);
/* a fresh TxFlow: forget every TxVoteSet and its tx id (TxVoteSets = make(map...) in NewTxFlow,
 * txflow/service.go:71), keeping the validator set and its tables */
int txv_reset_flow(txv_ctx* ctx);
int txv_sync(txv_ctx* ctx);
/* bind the calling thread and the library's host pack threads to the CPUs of the NUMA node the
 * GPU is attached to (sysfs local_cpulist), so the pinned batch buffers and the pack run next to
 * the GPU's PCIe root; TXV_ESTATE when the locality is unknown or no such CPU is allowed */
int txv_bind_host_numa(txv_ctx* ctx);

/* ---- TxVotePool ingest (txvotepool/txvotepool.go) ----
 * Long signatures: txv_votes.sig holds the first 64 bytes of each signature.  Calls taking
 * sig_full / sig_full_off (optional) read signature i from sig_full + sig_full_off[i]
 * (sig_len[i] bytes) when sig_len[i] > 64; without them such a vote is TXV_EINVAL. */

/* txVoteKey for n votes: keys_out[i] (32 bytes) = SHA-256(Signature_i), hashed on the GPU
 * (signatures > 64 bytes on the host). */
int txv_sig_keys(txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full, const uint64_t* sig_full_off,
                 uint8_t* keys_out);

typedef struct {
  uint32_t size;            /* MempoolConfig.Size: max txs in the pool (0 -> 5000, tendermint default) */
  uint32_t cache_size;      /* MempoolConfig.CacheSize: LRU entries; 0 -> 10000; TXV_POOL_NO_CACHE = nopTxCache */
  uint64_t max_txs_bytes;   /* MempoolConfig.MaxTxsBytes (0 -> 1 GiB) */
  uint32_t max_msg_bytes;   /* MempoolConfig.MaxMsgBytes (0 -> 1 MiB); max tx size = this - 8 (reactor.go:379) */
  uint32_t flags;           /* TXV_POOL_WAL: the pool writes a WAL (InitWAL, node/node.go:805-807);
                               TXV_POOL_DEVICE_CACHE: see below */
} txv_pool_config;
#define TXV_POOL_WAL 0x1u
/* The LRU cache (mapTxCache, txvotepool.go:416-438) kept in the HBM of the GPU of the context that
 * txv_pool_check, txv_pool_check_keys (with a ctx) and the wire ingest pass, where each batch's
 * CheckTx decisions are made in parallel (LRU stack distance: the decisions of the sequential loop)
 * and the new cache is built; the statuses come back and the admitted votes are appended to the
 * pool list (txs, txsMap) on the host within the same call.  A batch in which the Size or
 * MaxTxsBytes cap could bind, or (txv_pool_check) holding a signature longer than 64 bytes, runs on
 * the host as without the flag, as do Update and txv_pool_check_keys without a ctx: the cache list
 * is fetched back first and uploaded again by the next device batch.  The device copy is freed with
 * the pool. */
#define TXV_POOL_DEVICE_CACHE 0x2u
/* The pool keeps MempoolTxVote.Senders (txvotepool.go:364-371) for every entry of its list: see
 * "CheckTxWithInfo's senders" below.  Without the flag nothing is kept, no memory is allocated, no
 * kernel is enqueued and every call behaves as before.  With TXV_POOL_DEVICE_CACHE the sets live in
 * HBM beside the pool list, are written by each device batch's engine chain, and move between host
 * and device with the list. */
#define TXV_POOL_SENDERS 0x4u
#define TXV_POOL_NO_CACHE 0xFFFFFFFFu
typedef struct txv_pool txv_pool;

/* per-vote CheckTx results (nil error / the reference's error values) */
#define TXV_POOL_OK 0            /* added to the pool (nil) */
#define TXV_POOL_ERR_FULL 1      /* mempool.ErrMempoolIsFull */
#define TXV_POOL_ERR_TOO_LARGE 2 /* ErrTxTooLarge */
#define TXV_POOL_ERR_IN_CACHE 3  /* mempool.ErrTxInCache */
#define TXV_POOL_ERR_ENCODING 4  /* only with TXV_POOL_WAL: amino rejects the timestamp, so the WAL write's
                                    MustMarshalBinaryBare panics (txvotepool.go:231-242) after the
                                    cache push.  Without a WAL such a vote is admitted with
                                    TxVote.Size() == 0 (types/tx_vote.go:144-150) */

int  txv_pool_new(const txv_pool_config* cfg, int64_t height, txv_pool** out);
void txv_pool_free(txv_pool* pool);
/* CheckTxWithInfo for each vote in arrival order (keys on ctx's GPU); status_out[i] = TXV_POOL_*. */
int txv_pool_check(txv_pool* pool, txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full,
                   const uint64_t* sig_full_off, uint8_t* status_out);
/* txv_pool_check in two calls: submit (CheckTx'd in submission order; with TXV_POOL_DEVICE_CACHE
 * the keys, decisions and new cache are enqueued on the GPU and the call returns, so batch k+1
 * can be submitted while batch k's statuses are awaited; otherwise the batch is checked on the
 * host within the call) and wait (status_out[i] = TXV_POOL_*, any order).  A device batch's
 * registered signature columns are DMA'd from caller memory: they must stay valid until its
 * wait.  txv_pool_check = submit + wait.  txvotepool.go:187-261 */
int txv_pool_check_submit(txv_pool* pool, txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full,
                          const uint64_t* sig_full_off, uint64_t* ticket);
int txv_pool_check_wait(txv_pool* pool, uint64_t ticket, uint8_t* status_out);
/* TryAddVote for the batch pool_ticket (txv_pool_check_submit on the same batch) is deciding, as
 * the reactor hands CheckTx's accepted votes to checkMaj23Routine (txvotepool/reactor.go:170-190 ->
 * txflow/service.go:123-166): like txv_submit_votes (ticket for txv_wait_votes), the votes the
 * pool did not admit as nil entries.  While the CheckTx batch is still in the pool engine's flight
 * slot (TXV_POOL_DEVICE_CACHE) the AddVote chain is enqueued behind its decisions and reads its
 * statuses and already uploaded signatures in HBM: the call does not wait for them; otherwise
 * the ticket's statuses are taken on the host.  votes->is_nil, if given, is or-ed in.  The pool
 * ticket is still waited by the caller (txv_pool_check_wait, before or after this call).  Takes
 * the pool's lock, then the context's. */
int txv_submit_checked(txv_ctx* ctx, const txv_votes* votes, txv_pool* pool, uint64_t pool_ticket, uint64_t* ticket);
/* ---- CheckTx and TryAddVote from a route buffer in HBM: a validator's own votes stay on the device ----
 * <- txVotePool.CheckTx(txVote) of signTxRoutine (txvotepool/reactor.go:126 -> txvotepool.go:180-261)
 * for every vote of a route buffer in ctx's HBM (what txv_sign_txs_submit wrote, or any buffer of
 * the txv_route_admitted layout), in buffer order.  The pool ticket is an ordinary one:
 * txv_pool_check_wait collects it, it orders with every other CheckTx and Update submission, and
 * txv_pool_update_fired, txv_pool_sync, reap and the cache reads behave as after
 * txv_pool_check_submit.  Statuses and pool state equal txv_pool_check on the txv_route_view of a
 * host copy of the buffer, but for two classes of vote that call refuses wholesale and a buffer in
 * HBM cannot be inspected for before the submit returns; both get TXV_POOL_NOT_CHECKED and never
 * touch the pool: a vote whose TXV_ROUTE_NIL byte is set (a nil *TxVote never reaches CheckTx) and
 * a vote with sig_len > 64 (the buffer carries only its first 64 bytes, so its key cannot be
 * formed).  addr_len > 20 is not special: CheckTx never looks at the address and Size() uses the
 * length as given.
 *
 * With TXV_POOL_DEVICE_CACHE, the engine on ctx's GPU and caps that cannot bind (n pushes of the
 * largest Size() a vote with max_txhash_len, a 20-byte address and a 64-byte signature can have,
 * beside the batches in flight) nothing waits for the GPU and nothing crosses the link: one kernel
 * reads the buffer into the keys, sizes and validity the engine decides from.  Every other pool
 * (no TXV_POOL_DEVICE_CACHE, an engine on another GPU, caps that may bind) reads the buffer
 * back -- one copy, the only case that blocks -- and runs the host admission; the results are the
 * same in every mode.
 *
 * The submit cannot read the buffer's header, so the kernel does: unless magic, n, arena_bytes,
 * flags, max_txhash_len and total bytes all equal the meta's it touches nothing beyond the header,
 * every vote is TXV_POOL_NOT_CHECKED, the pool is unchanged, and txv_pool_check_wait writes those
 * statuses and returns TXV_EINVAL (txv_last_error(ctx) says why).  A meta must still never describe
 * more bytes than the allocation holds.
 *
 * TXV_EINVAL from the call itself: a null argument, buf_dev not 16-byte aligned, meta->bytes !=
 * txv_route_bytes(meta->n, meta->arena_bytes, meta->flags), n > max_batch.  n == 0 is a valid empty
 * batch: a pool ticket with zero statuses.
 *
 * Ordering and lifetime: the kernel (and txv_submit_routed_checked's staging copies) are enqueued
 * behind any txv_sign_txs_submit chain of the same context that is still writing the buffer, so
 * sign_submit -> check_routed_submit -> submit_routed_checked may be issued back to back with
 * txv_sign_txs_meta's meta and the three waits may follow in any order.  The buffer must stay
 * unchanged until both the pool ticket and the flow ticket are waited (the rule of registered
 * memory in txv_pool_check_submit).  txv_sync, txv_reset_flow and txv_destroy wait for the kernels
 * in flight first. */
int txv_pool_check_routed_submit(txv_pool* pool, txv_ctx* ctx, const void* buf_dev, const txv_route_meta* meta,
                                 uint64_t* pool_ticket);
/* submit + txv_pool_check_wait */
int txv_pool_check_routed(txv_pool* pool, txv_ctx* ctx, const void* buf_dev, const txv_route_meta* meta,
                          uint8_t* status_out);
/* <- checkMaj23Routine -> TryAddVote (txflow/service.go:123-166) for the batch that pool_ticket
 * (txv_pool_check_routed_submit on the same buffer) is deciding: txv_submit_routed with the votes
 * the pool did not admit as nil entries, the counterpart of txv_submit_checked.  A txv_submit_votes
 * ticket for txv_wait_votes from the same submit ring (four in flight, TXV_ESTATE beyond); the
 * gossip, store and Update sinks see the batch as they see any other.  While the pool ticket is in
 * the engine's flight slot the columns are staged by device-to-device copies, the nil column is
 * built on the device from the slot's statuses (or-ed into the buffer's own nil column when it has
 * one) and the chain runs behind the decisions with no host round trip; otherwise the ticket's
 * statuses are taken on the host, as txv_submit_checked does (TXV_ESTATE for an unknown ticket,
 * TXV_EINVAL for a batch of another size).  On a ticket whose buffer failed the header check it
 * runs a batch of nil entries.  Takes the submit lock, then the pool's, then the context's.
 *
 * The flight slot of a routed ticket holds statuses but no signatures: txv_submit_checked and
 * txv_route_submit_checked given such a ticket take its statuses on the host and the signatures
 * from the caller's columns. */
int txv_submit_routed_checked(txv_ctx* ctx, const void* buf_dev, const txv_route_meta* meta, txv_pool* pool,
                              uint64_t pool_ticket, uint64_t* ticket);
/* CheckTxWithInfo for n votes given as (txVoteKey, TxVote.Size()) pairs in arrival order: keys32
 * n x 32 bytes (SHA-256(Signature), txvotepool.go:467-469), sizes[i] = Size() (0 when amino
 * rejects the timestamp); status_out[i] = TXV_POOL_*.  ctx (optional) lends its host workers;
 * with NULL a batch of >= 4096 votes runs its passes on worker threads of the pool's own
 * (TXV_HOST_THREADS, else min(16, cores)), created on the first such call.  txvotepool.go:187-261 */
int txv_pool_check_keys(txv_pool* pool, txv_ctx* ctx, const uint8_t* keys32, const uint32_t* sizes, uint32_t n,
                        uint8_t* status_out);
/* The order-independent half of txv_pool_check: keys_out [n][32] = txVoteKey (SHA-256(Signature),
 * on the GPU) and sizes_out [n] = TxVote.Size() (host workers, while the GPU hashes); reads and
 * writes no pool state, so batch k+1 may be prepared while txv_pool_check_keys admits batch k on
 * another thread.  txv_pool_prepare + txv_pool_check_keys = txv_pool_check.  txvotepool.go:187-261 */
int txv_pool_prepare(txv_pool* pool, txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full,
                     const uint64_t* sig_full_off, uint8_t* keys_out, uint32_t* sizes_out);
/* Update(height, committed): every committed vote's key is pushed to the cache, and the vote
 * leaves the pool if its key is there (txvotepool.go:329-359); applied when it returns.  With
 * TXV_POOL_DEVICE_CACHE the keys are pushed by the device engine behind the batches submitted
 * before, and the committed votes leave the pool list held in HBM there too; nothing is copied back
 * but the removal counts. */
int txv_pool_update(txv_pool* pool, txv_ctx* ctx, int64_t height, const txv_votes* committed,
                    const uint8_t* sig_full, const uint64_t* sig_full_off);
/* Update with the committed votes given as (txVoteKey, TxVote.Size()) pairs, as
 * txv_pool_check_keys takes them; applied when it returns, on the host (a pool list or cache held
 * in HBM comes back first).  ctx (optional) lends its host workers.  txvotepool.go:329-359 */
int txv_pool_update_keys(txv_pool* pool, txv_ctx* ctx, int64_t height, const uint8_t* keys32, const uint32_t* sizes,
                         uint32_t n);
/* txv_pool_update without the wait (the commit path of a node that keeps checking batches):
 * with TXV_POOL_DEVICE_CACHE it stages the committed votes (their signatures uploaded) and returns;
 * the staged pushes and removals are applied ahead of the NEXT device CheckTx batch submitted
 * (txv_pool_check_submit, txv_pool_check_keys with a context, the wire ingest), in that batch's
 * engine chain -- the reference's order: Update, then the CheckTx calls after it -- or alone at
 * txv_pool_sync, at any call that reads the pool list or cache, or when staged entries from
 * another context or too many for one flight would otherwise wait.  Waiting on tickets submitted
 * before the Update does not apply it.  The host cache applies it at once.
 * txflow/service.go:224-227 -> txvotepool.go:329-359 */
int txv_pool_update_submit(txv_pool* pool, txv_ctx* ctx, int64_t height, const txv_votes* committed,
                           const uint8_t* sig_full, const uint64_t* sig_full_off);
/* txv_pool_update_submit with the list ctx built on the device for the batch of `ticket` as
 * `committed` (txv_update_sink_enable; the ticket waited for): "apply the Update for what this
 * batch committed" without the host listing the votes.  With TXV_POOL_DEVICE_CACHE on ctx's
 * device the entries are copied device to device into the engine's pending slot -- no signature
 * crosses the link, the call waits for nothing -- and applied ahead of the next CheckTx batch, or
 * at txv_pool_sync (txv_pool_update_fired then txv_pool_sync: applied on return).  A pool with a
 * host cache, or an engine on another GPU, gets the list's keys (hashed on ctx's GPU) and sizes
 * and applies them at once.  An empty list only sets the height.  The errors of txv_update_list;
 * on any of them (TXV_ECAPACITY: the list overflowed the sink) the pool is unchanged.
 * txflow/service.go:216-227 -> txvotepool.go:329-359 */
int txv_pool_update_fired(txv_pool* pool, txv_ctx* ctx, int64_t height, uint64_t ticket);
/* ReapMaxTxs(max) in pool order: keys (32 B) and TxVote.Size of the reaped entries; the
 * reference loop condition `len(txs) <= max` reaps max + 1 entries when available; max < 0 = all.
 * keys_out / sizes_out capacity `cap`; *n_out = entries reaped (may exceed cap: truncated). */
int txv_pool_reap(txv_pool* pool, int64_t max, uint8_t* keys_out, uint32_t* sizes_out, uint64_t cap,
                  uint64_t* n_out);
/* Flush: empty pool and cache. */
int txv_pool_flush(txv_pool* pool);
int64_t txv_pool_size(txv_pool* pool);
int64_t txv_pool_txs_bytes(txv_pool* pool);
int64_t txv_pool_height(txv_pool* pool);
/* With TXV_POOL_DEVICE_CACHE the pool list lives in HBM beside the cache: a device batch's engine
 * chain appends the votes it admitted and removes an Update's committed ones in submission order
 * (there is no appender thread); Size and TxsBytes follow each finished batch's counts, and every
 * call that reads the pool list or cache finishes the submitted batches first.  txv_pool_sync
 * applies the Updates submitted so far (txv_pool_update_submit, txv_pool_update_fired): staged
 * entries are decided and every submitted batch up to them finished.  Call it before txv_destroy
 * of the context the pool last ran on when the pool outlives it (txv_pool_free waits too). */
int txv_pool_sync(txv_pool* pool);
/* LRU cache keys front (oldest) to back; *n_out = cache length (test hook: cache_test.go). */
int txv_pool_cache_keys(txv_pool* pool, uint8_t* keys_out, uint64_t cap, uint64_t* n_out);

/* ---- CheckTxWithInfo's senders (TXV_POOL_SENDERS) ----
 * CheckTxWithInfo(tx, cb, TxInfo{SenderID}) differs from CheckTx in one thing: the pool entry
 * remembers which peers sent the vote (MempoolTxVote.Senders), so broadcastTxRoutine does not send
 * it back to them (txvotepool/reactor.go:245).  For each vote of a batch in arrival order, with
 * sender id s (0 = UnknownPeerID):
 *   TXV_POOL_OK            the new entry's set is {s}                               (:250)
 *   TXV_POOL_ERR_IN_CACHE  if txsMap holds the vote's key at that moment, s joins that entry's
 *                          set; otherwise nothing (a committed vote is cached, not pooled) (:213-227)
 *   every other status     nothing (ERR_ENCODING is returned before addTx: no entry exists)
 * Update's committed votes remove entries together with their sets and record no sender;
 * txv_pool_flush empties all sets.  The calls without a sender argument (txv_pool_check*,
 * txv_pool_check_routed*, txv_pool_receive, txv_ingest_*) record sender 0, as CheckTx does
 * (:180-182).  "At that moment" holds inside a batch too: a key admitted, hit, evicted from the
 * cache, admitted again and hit again within one batch leaves the first hit's sender with the
 * first entry and the second's with the second (the one txsMap indexes afterwards).
 * The *_from calls are their namesakes with a sender column: senders == NULL = all 0; senders[i]
 * is read even for a vote that ends up not checked; on a pool without TXV_POOL_SENDERS a non-NULL
 * column returns TXV_ESTATE and touches nothing.  txv_ingest_decode_from copies the column before
 * it returns; the ticket's admit (txv_ingest_admit, or the _admit_submit / _admit_finish pair)
 * uses it.
 * txv_pool_sent_by: bits_out = [n][ceil(n_peers / 32)] words; bit p of row i is set iff txsMap holds
 *   key i now -- after every batch and Update submitted so far, which the call finishes first, as
 *   every reader of the pool list does -- and peers[p] is in that entry's Senders.  A key not in
 *   the pool gives a zero row.  ctx is optional, as for txv_pool_check_keys.  TXV_ESTATE without
 *   the flag, TXV_EINVAL for null arguments or n_peers == 0.  Takes the pool's lock, then the
 *   context's (the order of txv_submit_checked).
 * txv_pool_ticket_sent_by: the same rows for the votes of a CheckTx ticket, with the keys read
 *   where they lie in the device engine's flight slot (only the rows of votes the ticket admitted
 *   are filled; a row is looked up by key, so a vote re-admitted later under the same key reports
 *   the later entry, as txsMap.Load does).  The call finishes the ticket, and every batch
 *   submitted so far, first.  TXV_ESTATE when the ticket no longer holds its flight slot (eight
 *   later batches have taken the ring's slots), was decided on the host, or is a routed batch
 *   (its keys were never in the slot): the caller then uses the key form.  This is what a node on
 *   the device path calls before it gossips a batch: it never sees keys.
 * txv_pool_senders_stats (test hook): stats_out = {words stored in the set, those of entries
 *   that left the list included (in HBM: the host's upper bound); slots; rebuilds of the set so
 *   far; compactions of the list in HBM so far; 1 when the list and its sets are in HBM now}. */
int txv_pool_check_submit_from(txv_pool* pool, txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full,
                               const uint64_t* sig_full_off, const uint16_t* senders, uint64_t* ticket);
int txv_pool_check_from(txv_pool* pool, txv_ctx* ctx, const txv_votes* votes, const uint8_t* sig_full,
                        const uint64_t* sig_full_off, const uint16_t* senders, uint8_t* status_out);
int txv_pool_check_keys_from(txv_pool* pool, txv_ctx* ctx, const uint8_t* keys32, const uint32_t* sizes, uint32_t n,
                             const uint16_t* senders, uint8_t* status_out);
int txv_pool_sent_by(txv_pool* pool, txv_ctx* ctx, const uint8_t* keys32, uint32_t n, const uint16_t* peers,
                     uint32_t n_peers, uint32_t* bits_out);
int txv_pool_ticket_sent_by(txv_pool* pool, txv_ctx* ctx, uint64_t pool_ticket, const uint16_t* peers,
                            uint32_t n_peers, uint32_t* bits_out);
int txv_pool_senders_stats(txv_pool* pool, uint64_t stats_out[5]);

/* ---- TxVoteMessage wire decode (Reactor.Receive, txvotepool/reactor.go:170-190, 273-291) ----
 * n received messages (message i = wire[msg_off[i] .. + msg_len[i]), wire < 4 GiB) decoded on
 * the GPU, amino UnmarshalBinaryBare of the TxpoolMessage interface whose one registered
 * concrete is &TxVoteMessage{Tx types.TxVote} ("tendermint/txvotepool/TxVoteMessage"), straight
 * into the txv_votes layout.  TxHash bytes and signatures stay in the caller's buffer:
 * txhash_off / sig_off index `wire`, so txv_votes{txhash = wire, txhash_off, ...} with
 * sig_full = wire, sig_full_off = sig_off feeds txv_pool_check / txv_add_votes directly. */
#define TXV_WIRE_OK 0          /* *TxVoteMessage -> CheckTxWithInfo(msg.Tx) */
#define TXV_WIRE_TOO_LARGE 1   /* len > MaxMsgBytes: decodeMsg's ErrTxTooLarge (peer stopped) */
#define TXV_WIRE_ERR_DECODE 2  /* amino decode error (peer stopped) */
#define TXV_WIRE_NIL 3         /* empty message: nil msg, "Unknown message type" (ignored) */
typedef struct {             /* caller-owned [n] arrays; any pointer may be NULL (not written) */
  uint8_t*  status;          /* TXV_WIRE_*; the fields below are zero unless TXV_WIRE_OK */
  int64_t*  height;
  uint32_t* txhash_off;      /* TxHash bytes at wire + txhash_off */
  uint32_t* txhash_len;
  uint8_t*  txkey;           /* [n][32] TxKey */
  int64_t*  ts_sec;          /* Timestamp (absent = the Unix epoch, amino's default time) */
  int32_t*  ts_nanos;
  uint8_t*  addr;            /* [n][20] first 20 bytes of ValidatorAddress, zero beyond its length */
  uint32_t* addr_len;
  uint8_t*  sig;             /* [n][64] first 64 bytes of Signature, zero beyond its length */
  uint32_t* sig_len;
  uint64_t* sig_off;         /* Signature bytes at wire + sig_off */
} txv_wire_votes;
int txv_decode_msgs(txv_ctx* ctx, const uint8_t* wire, uint64_t wire_bytes, const uint64_t* msg_off,
                    const uint32_t* msg_len, uint32_t n, uint32_t max_msg_bytes, const txv_wire_votes* out);
/* the same in three steps (bench / pipelining): upload, decode `reps` times on the device
 * (average kernel time), copy the results of the last run out */
int txv_decode_stage(txv_ctx* ctx, const uint8_t* wire, uint64_t wire_bytes, const uint64_t* msg_off,
                     const uint32_t* msg_len, uint32_t n);
int txv_decode_run(txv_ctx* ctx, uint32_t max_msg_bytes, uint32_t reps, float* kernel_ms_avg);
int txv_decode_fetch(txv_ctx* ctx, const txv_wire_votes* out);
/* Reactor.Receive for n messages in arrival order: decode (GPU) with the pool's MaxMsgBytes, then
 * CheckTxWithInfo for every decoded TxVoteMessage.  wire_status_out[i] = TXV_WIRE_*;
 * pool_status_out[i] = TXV_POOL_* for TXV_WIRE_OK messages, TXV_POOL_NOT_CHECKED otherwise. */
#define TXV_POOL_NOT_CHECKED 0xFF
/* the sending side, broadcastTxRoutine's cdc.MustMarshalBinaryBare(&TxVoteMessage{tx})
 * (txvotepool/reactor.go:248), for a batch on host threads: message i at out + off_out[i],
 * len_out[i] bytes; txkey [n][32] or NULL (zero TxKey); signatures > 64 bytes from sig_full +
 * sig_full_off[i].  Nil votes, addresses > 20 bytes and times amino rejects (the reference panics)
 * are TXV_EINVAL.  *bytes_out = total size; TXV_ECAPACITY (nothing written) when it exceeds cap. */
int txv_encode_msgs(const txv_votes* votes, const uint8_t* txkey, const uint8_t* sig_full,
                    const uint64_t* sig_full_off, uint8_t* out, uint64_t cap, uint64_t* off_out, uint32_t* len_out,
                    uint64_t* bytes_out);
int txv_pool_receive(txv_pool* pool, txv_ctx* ctx, const uint8_t* wire, uint64_t wire_bytes,
                     const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, uint8_t* wire_status_out,
                     uint8_t* pool_status_out);
/* txv_pool_receive with senders[i] = the id of the peer message i came from (Receive's
 * txInfo.SenderID, reactor.go:183-188); "CheckTxWithInfo's senders" above */
int txv_pool_receive_from(txv_pool* pool, txv_ctx* ctx, const uint8_t* wire, uint64_t wire_bytes,
                          const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, const uint16_t* senders,
                          uint8_t* wire_status_out, uint8_t* pool_status_out);
/* The whole ingest chain for n received messages in arrival order, device-resident:
 *   Reactor.Receive / decodeMsg (txvotepool/reactor.go:170-190, 278-284)
 *   -> TxVotePool.CheckTxWithInfo (txvotepool/txvotepool.go:187-261) for every decoded vote
 *   -> TxFlow.TryAddVote (txflow/service.go:169-234) for every vote the pool admitted, in order
 * (the order the reference's checkMaj23Routine walks the pool's list, service.go:123-166).
 * The wire bytes are uploaded once; the decoded votes stay in HBM: the pool's keys
 * (SHA-256(Signature)) and TxVote.Size() are computed on the device and only they cross back
 * for the order-dependent LRU admission; the admitted votes' TxVote columns are built on the
 * device from the decoded records and run through the AddVote chain of txv_add_votes.
 * wire_status[i] = TXV_WIRE_*; pool_status[i] = TXV_POOL_* (TXV_POOL_NOT_CHECKED when not
 * decoded); flow_status[i] = txv_add_votes' status (| TXV_STATUS_FIRED) for admitted votes,
 * TXV_FLOW_NOT_ADDED otherwise; commit events (up to ev_cap; *n_ev = total) carry the MESSAGE
 * index as vote_index.  Any output pointer may be NULL.  = txv_ingest_submit + txv_ingest_wait.
 * A failure after the pool stage (e.g. a TxFlow capacity overflow, TXV_ECAPACITY) is returned with
 * every pool-admitted vote's flow_status = TXV_FLOW_NOT_RUN: those votes are in the pool (a resent
 * message is ErrTxInCache) but not in TxFlow; the caller re-feeds them through txv_add_votes
 * (e.g. from txv_decode_msgs' columns) after txv_reset_flow. */
#define TXV_FLOW_NOT_ADDED 0xFE
#define TXV_FLOW_NOT_RUN 0xFD
int txv_ingest_msgs(txv_ctx* ctx, txv_pool* pool, const uint8_t* wire, uint64_t wire_bytes,
                    const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, uint8_t* wire_status,
                    uint8_t* pool_status, uint8_t* flow_status, txv_commit_event* ev_out, uint32_t ev_cap,
                    uint32_t* n_ev);
/* txv_ingest_msgs split for pipelining (Reactor.Receive -> CheckTxWithInfo -> checkMaj23Routine's
 * TryAddVote, txvotepool/reactor.go:170-190 -> txvotepool.go:187-261 -> txflow/service.go:123-166,
 * as the reference's goroutines overlap them): txv_ingest_submit uploads and decodes the batch
 * on the GPU, runs CheckTxWithInfo for its decoded votes on the host (wire_status / pool_status
 * are final when it returns) and enqueues the admitted votes' AddVote chain without waiting for
 * it; txv_ingest_wait(ticket) waits for that chain and reports flow_status [n] and the commit
 * events as txv_ingest_msgs does.  At most three ingest batches in flight, waited in submission
 * order; submits are serialised among themselves (pool order = TxFlow order), but the context is
 * not locked during a submit's pool stage, so AddVote batches (txv_submit_votes / txv_wait_votes)
 * and ingest waits of other threads proceed meanwhile.  The caller's buffers may be reused once
 * txv_ingest_submit returns.  An error before the pool stage returns without a ticket and leaves
 * the pool unchanged; once the pool admitted votes the submit returns a ticket, and a failure of
 * the TxFlow stage is returned by the wait with TXV_FLOW_NOT_RUN as above. */
int txv_ingest_submit(txv_ctx* ctx, txv_pool* pool, const uint8_t* wire, uint64_t wire_bytes,
                      const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, uint8_t* wire_status,
                      uint8_t* pool_status, uint64_t* ticket);
/* txv_ingest_submit in its two halves, for a third pipeline stage (a node's Receive goroutine
 * decoding the next batch while the previous one is in CheckTx): txv_ingest_decode uploads the
 * batch (wire bytes inside memory registered with txv_host_register are DMA'd from there, and
 * read until the batch's txv_ingest_admit returns; other buffers may be reused at once), decodes
 * it and starts its keys' copy back, returning a ticket without waiting; txv_ingest_admit(ticket)
 * waits for the keys, runs CheckTxWithInfo and enqueues the TxFlow chain (wire_status /
 * pool_status [n] final on return).  Tickets are admitted in decode order, at most three batches
 * are between decode and wait; an error from txv_ingest_admit ends its ticket (the pool is
 * unchanged, no wait follows). */
int txv_ingest_decode(txv_ctx* ctx, txv_pool* pool, const uint8_t* wire, uint64_t wire_bytes,
                      const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, uint64_t* ticket);
int txv_ingest_admit(txv_ctx* ctx, uint64_t ticket, uint8_t* wire_status, uint8_t* pool_status);
/* txv_ingest_decode with the messages' peer ids ("CheckTxWithInfo's senders" above): the column is
 * copied before the call returns and used by the ticket's admit */
int txv_ingest_decode_from(txv_ctx* ctx, txv_pool* pool, const uint8_t* wire, uint64_t wire_bytes,
                           const uint64_t* msg_off, const uint32_t* msg_len, uint32_t n, const uint16_t* senders,
                           uint64_t* ticket);
/* txv_ingest_admit in its two halves, for a fourth stage (the admit thread waited for
 * each batch's pool statuses): txv_ingest_admit_submit hands the batch's CheckTx to the device (the
 * pool keeps its cache in HBM and the caps cannot bind: the decisions are enqueued behind the
 * decode in the pool engine's next flight slot) together with the batch's TxFlow chain over every
 * decoded message, the pool's rejections and the undecodable messages as nil entries built on the
 * device from those decisions (messages of up to 1024 bytes; a batch with a longer one has its
 * chain enqueued by the finish), and returns; txv_ingest_admit_finish (tickets in order) collects
 * the statuses and lists the admitted messages.
 * wire_status / pool_status are final when the finish returns (when the submit had to run the
 * host path, the whole admission is done by the submit -- it requires every earlier submitted
 * admission finished, else TXV_ESTATE -- and the finish returns at once).  A registered wire
 * buffer is read until the finish returns. */
int txv_ingest_admit_submit(txv_ctx* ctx, uint64_t ticket, uint8_t* wire_status, uint8_t* pool_status);
int txv_ingest_admit_finish(txv_ctx* ctx, uint64_t ticket, uint8_t* wire_status, uint8_t* pool_status);
int txv_ingest_wait(txv_ctx* ctx, uint64_t ticket, uint8_t* flow_status, txv_commit_event* ev_out, uint32_t ev_cap,
                    uint32_t* n_ev);

/* ---- self-test hook: field/scalar ops on device (tests only) ----
 * a, b, out: n x 8 little-endian u32 words.  op:
 *   0 a*b   1 a^2   2 a+b   3 a-b   (radix-2^32 fe, weakly reduced results)
 *   4 canon(a)   5 fe_invert(a)   6 sc_reduce512(a || b)   7 fe_invert_var(a) (canonical)
 *   8 fe_from_fe10(fe10_mul(4 x10, 3 y10)) with x10 = fe10_strict(fe10_from_fe(a)), y10 of b, the
 *     multiples built by fe10_add: the walk's multiply at its documented operand bounds
 *   9, 10 the first / second product of fe10_mul2(4 x10, 3 y10, 3 y10, 3 x10), likewise
 * Any other op: TXV_EINVAL. */
int txv_fe_selftest(txv_ctx* ctx, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t n, int op);

#ifdef __cplusplus
}
#endif
#endif
