package pbftv

/*
#include "pbftv.h"
*/
import "C"

// Sealing (include/pbftv.h "Sealing"): what a replica posts -- the Go struct
// plus "signature":"<base64>" -- for a whole batch of votes, replies or
// pre-prepares in one GPU round trip: json.Marshal of the unsigned struct,
// SHA-256, the RFC 6979 signature under a registered signing key, and the
// signed wire JSON, every message's bytes back to back in one buffer.  The
// bytes are json.Marshal's of the signed struct: json.Unmarshal reads them.

// ENOSPACE: the sealed batch did not fit the buffer handed in.
const ENOSPACE = -7

// SigFormat selects the bytes of the Signature field.
type SigFormat int

const (
	SigRS  SigFormat = 0 // r||s, 64 bytes
	SigDER SigFormat = 1 // what ecdsa.SignASN1 writes
)

// Sealed is a sealed batch: message i is Wire[Off[i] : Off[i]+Len[i]]; a
// message that was not signed (OK[i] false: key index out of range, invalid
// key) has length 0.
type Sealed struct {
	Wire    []byte
	Off     []uint64
	Len     []uint32
	Digests [][32]byte // SHA-256(json.Marshal(unsigned message)): what was signed
	OK      []bool
}

// Message returns message i's wire JSON (nil if it was not signed).
func (s *Sealed) Message(i int) []byte {
	if s.Len[i] == 0 {
		return nil
	}
	return s.Wire[s.Off[i] : s.Off[i]+uint64(s.Len[i]) : s.Off[i]+uint64(s.Len[i])]
}

func sigTail(f SigFormat) int {
	if f == SigDER {
		return 111
	}
	return 103
}

// newSealed allocates the outputs: wireCap is the header's upper bound for the
// batch, so no call returns ENOSPACE.
func newSealed(n, wireCap int) (*Sealed, []byte, C.uint64_t) {
	return &Sealed{Wire: make([]byte, wireCap+1), Off: make([]uint64, n), Len: make([]uint32, n),
		Digests: make([][32]byte, n)}, make([]byte, (n+7)/8+1), 0
}

func (s *Sealed) finish(bm []byte, total C.uint64_t) *Sealed {
	s.Wire = s.Wire[:int(total)]
	s.OK = bits(bm, len(s.Len))
	return s
}

// SealVotes signs and encodes a snapshot of outgoing prepare / commit votes
// (pbftv_seal_votes): the sender's side of FlushVotes.
func (x *Ctx) SealVotes(votes []VoteMsg, keyIdx []uint32, format SigFormat) (*Sealed, error) {
	n := len(votes)
	if len(keyIdx) != n {
		return nil, &Error{Code: EINVAL, Msg: "column lengths differ"}
	}
	if n == 0 {
		return &Sealed{}, nil
	}
	views, seqs, types := make([]int64, n), make([]int64, n), make([]int64, n)
	dg, ids := make([]string, n), make([]string, n)
	bound := 0
	for i, v := range votes {
		views[i], seqs[i], types[i] = v.ViewID, v.SequenceID, int64(v.MsgType)
		dg[i], ids[i] = v.Digest, v.NodeID
		bound += 120 + 6*(len(v.Digest)+len(v.NodeID)) + sigTail(format)
	}
	d, id := packStrings(dg), packStrings(ids)
	s, bm, total := newSealed(n, bound)
	err := call(func() C.int { return C.pbftv_seal_votes(x.c, C.uint64_t(n), i64(views), i64(seqs), u8(d.blob), u64(d.off), u32(d.ln),
		u8(id.blob), u64(id.off), u32(id.ln), i64(types), u32(keyIdx), C.int(format), u8(s.Wire), C.uint64_t(bound),
		u64(s.Off), u32(s.Len), &total, digestPtr(s.Digests), u8(bm)) })
	if err != nil {
		return nil, err
	}
	return s.finish(bm, total), nil
}

// SealReplies signs and encodes a batch of replies (pbftv_seal_replies): the
// sender's side of FlushReplies.
func (x *Ctx) SealReplies(reps []ReplyMsg, keyIdx []uint32, format SigFormat) (*Sealed, error) {
	n := len(reps)
	if len(keyIdx) != n {
		return nil, &Error{Code: EINVAL, Msg: "column lengths differ"}
	}
	if n == 0 {
		return &Sealed{}, nil
	}
	views, ts, cid, id, rs := replyColumns(reps)
	bound := 0
	for _, r := range reps {
		bound += 102 + 6*(len(r.ClientID)+len(r.NodeID)+len(r.Result)) + sigTail(format)
	}
	s, bm, total := newSealed(n, bound)
	err := call(func() C.int { return C.pbftv_seal_replies(x.c, C.uint64_t(n), i64(views), i64(ts), u8(cid.blob), u64(cid.off), u32(cid.ln),
		u8(id.blob), u64(id.off), u32(id.ln), u8(rs.blob), u64(rs.off), u32(rs.ln), u32(keyIdx), C.int(format),
		u8(s.Wire), C.uint64_t(bound), u64(s.Off), u32(s.Len), &total, digestPtr(s.Digests), u8(bm)) })
	if err != nil {
		return nil, err
	}
	return s.finish(bm, total), nil
}

// SealPrePrepares signs and encodes the primary's pre-prepares
// (pbftv_seal_preprepares).  reqSigs[i] is the client's signature the embedded
// request carries on the wire, as it arrived: nil is Go's nil slice (written
// null), an empty non-nil slice is written "".  reqSigs == nil: all nil.
func (x *Ctx) SealPrePrepares(pps []PrePrepareMsg, reqSigs [][]byte, keyIdx []uint32, format SigFormat) (*Sealed, error) {
	n := len(pps)
	if len(keyIdx) != n || (reqSigs != nil && len(reqSigs) != n) {
		return nil, &Error{Code: EINVAL, Msg: "column lengths differ"}
	}
	if n == 0 {
		return &Sealed{}, nil
	}
	views, seqs, rts, rseqs := make([]int64, n), make([]int64, n), make([]int64, n), make([]int64, n)
	has, rnil := make([]byte, n+1), make([]byte, n+1)
	dg, cids, ops := make([]string, n), make([]string, n), make([]string, n)
	bound := 0
	for i, p := range pps {
		views[i], seqs[i], dg[i] = p.ViewID, p.SequenceID, p.Digest
		bound += 189 + 6*len(p.Digest) + sigTail(format) + 15
		if p.RequestMsg != nil {
			has[i] = 1
			rts[i], rseqs[i] = p.RequestMsg.Timestamp, p.RequestMsg.SequenceID
			cids[i], ops[i] = p.RequestMsg.ClientID, p.RequestMsg.Operation
			bound += 6 * (len(cids[i]) + len(ops[i]))
		}
		if reqSigs == nil || reqSigs[i] == nil {
			rnil[i] = 1
		} else {
			bound += 4 * ((len(reqSigs[i]) + 2) / 3)
		}
	}
	d, cid, op := packStrings(dg), packStrings(cids), packStrings(ops)
	var rsig column
	var rsBlob, rsNil *C.uint8_t
	if reqSigs != nil {
		rsig = packBytes(reqSigs)
		rsBlob, rsNil = u8(rsig.blob), u8(rnil)
		if rsBlob == nil { // every signature empty: the column is still there
			rsBlob = u8(make([]byte, 1))
		}
	}
	s, bm, total := newSealed(n, bound)
	err := call(func() C.int { return C.pbftv_seal_preprepares(x.c, C.uint64_t(n), i64(views), i64(seqs), u8(d.blob), u64(d.off), u32(d.ln),
		u8(has), i64(rts), u8(cid.blob), u64(cid.off), u32(cid.ln), u8(op.blob), u64(op.off), u32(op.ln), i64(rseqs),
		rsBlob, u64(rsig.off), u32(rsig.ln), rsNil, u32(keyIdx), C.int(format), u8(s.Wire), C.uint64_t(bound),
		u64(s.Off), u32(s.Len), &total, digestPtr(s.Digests), u8(bm)) })
	if err != nil {
		return nil, err
	}
	return s.finish(bm, total), nil
}
