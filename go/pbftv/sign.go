package pbftv

/*
#include "pbftv.h"
*/
import "C"

import "unsafe"

// Signing (include/pbftv.h "Signing"): what a replica sends it signs in one
// GPU round trip per batch.  The signatures are crypto/ecdsa.Sign's over a
// 32-byte digest with the nonce of RFC 6979 (deterministic: the same digest
// and key always give the same signature; no low-S normalisation, as in Go),
// so ecdsa.Verify and every verify of this package accept them.
//
// The signing keys are a set of their own: RegisterSigningKeys does not touch
// the public keys of RegisterKeys.  The library keeps the private keys in
// device memory only, overwrites them with zeros when the set is replaced and
// when the context closes, and never copies one back.  The nonce's digits
// address the G table on the GPU: the GPU and whoever shares it are trusted.

// ENOSIGNKEYS: a sign call before RegisterSigningKeys.
const ENOSIGNKEYS = -6

// RegisterSigningKeys replaces the context's signing keys with priv (D of an
// ecdsa.PrivateKey as 32 big-endian bytes: D.FillBytes); valid[j] is false for
// d = 0 or d >= n, and such a key signs nothing.
func (x *Ctx) RegisterSigningKeys(priv [][32]byte) ([]bool, error) {
	valid := make([]byte, len(priv)+1)
	var p *C.uint8_t
	if len(priv) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&priv[0]))
	}
	if err := call(func() C.int { return C.pbftv_register_signing_keys(x.c, p, C.uint32_t(len(priv)), u8(valid)) }); err != nil {
		return nil, err
	}
	out := make([]bool, len(priv))
	for i := range out {
		out[i] = valid[i] == 1
	}
	return out, nil
}

// SignBatch signs hashes[i] under signing key keyIdx[i]: sigs[i] = r||s
// big-endian, what VerifySigs takes.  ok[i] is false, and sigs[i] all zero,
// where keyIdx[i] is out of range or names an invalid key.
func (x *Ctx) SignBatch(hashes [][32]byte, keyIdx []uint32) (sigs [][64]byte, ok []bool, err error) {
	n := len(hashes)
	if len(keyIdx) != n {
		return nil, nil, &Error{Code: EINVAL, Msg: "hashes and keyIdx differ in length"}
	}
	if n == 0 {
		return nil, nil, nil
	}
	sigs = make([][64]byte, n)
	bm := make([]byte, (n+7)/8+1)
	err = call(func() C.int { return C.pbftv_ecdsa_p256_sign_batch(x.c, digestPtr(hashes), u32(keyIdx), C.uint64_t(n), sigPtr(sigs), u8(bm)) })
	if err != nil {
		return nil, nil, err
	}
	return sigs, bits(bm, n), nil
}

// derSlots cuts the library's 72-byte slots to their lengths; nil = not signed.
func derSlots(slots []byte, lens []uint32) [][]byte {
	out := make([][]byte, len(lens))
	for i, l := range lens {
		if l > 0 {
			out[i] = slots[72*i : 72*i+int(l) : 72*i+int(l)]
		}
	}
	return out
}

// SignBatchASN1 is SignBatch with the signatures as ecdsa.SignASN1 encodes
// them (what ecdsa.VerifyASN1 and VerifySigsASN1 take); nil where not signed.
func (x *Ctx) SignBatchASN1(hashes [][32]byte, keyIdx []uint32) ([][]byte, error) {
	n := len(hashes)
	if len(keyIdx) != n {
		return nil, &Error{Code: EINVAL, Msg: "hashes and keyIdx differ in length"}
	}
	if n == 0 {
		return nil, nil
	}
	slots, lens := make([]byte, 72*n), make([]uint32, n)
	err := call(func() C.int { return C.pbftv_ecdsa_p256_sign_der_batch(x.c, digestPtr(hashes), u32(keyIdx), C.uint64_t(n), u8(slots), u32(lens)) })
	if err != nil {
		return nil, err
	}
	return derSlots(slots, lens), nil
}

func replyColumns(reps []ReplyMsg) (views, ts []int64, cid, id, rs column) {
	n := len(reps)
	views, ts = make([]int64, n), make([]int64, n)
	cids, ids, results := make([]string, n), make([]string, n), make([]string, n)
	for i, r := range reps {
		views[i], ts[i], cids[i], ids[i], results[i] = r.ViewID, r.Timestamp, r.ClientID, r.NodeID, r.Result
	}
	return views, ts, packStrings(cids), packStrings(ids), packStrings(results)
}

// SignReplies digests and signs a batch of replies in one round trip: the
// replica's side of FlushReplies (json.Marshal, SHA-256 and ecdsa.Sign of
// every reply, the digests never leaving the GPU in between).  SealReplies /
// SealVotes (seal.go) return the signed wire JSON instead of bare signatures.
func (x *Ctx) SignReplies(reps []ReplyMsg, keyIdx []uint32) (digests [][32]byte, sigs [][64]byte, ok []bool, err error) {
	n := len(reps)
	if len(keyIdx) != n {
		return nil, nil, nil, &Error{Code: EINVAL, Msg: "column lengths differ"}
	}
	if n == 0 {
		return nil, nil, nil, nil
	}
	views, ts, cid, id, rs := replyColumns(reps)
	digests, sigs = make([][32]byte, n), make([][64]byte, n)
	bm := make([]byte, (n+7)/8+1)
	err = call(func() C.int { return C.pbftv_sign_replies(x.c, C.uint64_t(n), i64(views), i64(ts), u8(cid.blob), u64(cid.off), u32(cid.ln),
		u8(id.blob), u64(id.off), u32(id.ln), u8(rs.blob), u64(rs.off), u32(rs.ln), u32(keyIdx), digestPtr(digests),
		sigPtr(sigs), u8(bm)) })
	if err != nil {
		return nil, nil, nil, err
	}
	return digests, sigs, bits(bm, n), nil
}

// SignRepliesASN1 is SignReplies with DER signatures; nil where not signed.
func (x *Ctx) SignRepliesASN1(reps []ReplyMsg, keyIdx []uint32) (digests [][32]byte, sigs [][]byte, err error) {
	n := len(reps)
	if len(keyIdx) != n {
		return nil, nil, &Error{Code: EINVAL, Msg: "column lengths differ"}
	}
	if n == 0 {
		return nil, nil, nil
	}
	views, ts, cid, id, rs := replyColumns(reps)
	digests = make([][32]byte, n)
	slots, lens := make([]byte, 72*n), make([]uint32, n)
	err = call(func() C.int { return C.pbftv_sign_replies_der(x.c, C.uint64_t(n), i64(views), i64(ts), u8(cid.blob), u64(cid.off), u32(cid.ln),
		u8(id.blob), u64(id.off), u32(id.ln), u8(rs.blob), u64(rs.off), u32(rs.ln), u32(keyIdx), digestPtr(digests),
		u8(slots), u32(lens)) })
	if err != nil {
		return nil, nil, err
	}
	return digests, derSlots(slots, lens), nil
}
