package pbftv

// Sealing on the GPU against the standard library: every sealed message is
// what json.Marshal writes for the signed struct, json.Unmarshal reads it
// back, its signature is accepted by crypto/ecdsa under the matching public
// key and by this package's own flushes; a bad key index seals nothing.
// Skipped where pbftv_open finds no gfx950 device.
//
// NOTE: written without a Go toolchain at hand; it has not been compiled.

import (
	"bytes"
	"crypto/ecdsa"
	"crypto/sha256"
	"encoding/json"
	"math/big"
	"testing"
)

type signedVote struct {
	VoteMsg
	Signature []byte `json:"signature"`
}

type signedRequest struct {
	RequestMsg
	Signature []byte `json:"signature"`
}

type signedPrePrepare struct {
	ViewID     int64          `json:"viewID"`
	SequenceID int64          `json:"sequenceID"`
	Digest     string         `json:"digest"`
	RequestMsg *signedRequest `json:"requestMsg"`
	Signature  []byte         `json:"signature"`
}

func TestSealVotesAgainstStdlib(t *testing.T) {
	x := gpu(t)
	rfc, rfcPriv, rfcPub := signKey(t, rfcKey)
	other, otherPriv, otherPub := signKey(t, "0000000000000000000000000000000000000000000000000000000000000005")
	keys := []*ecdsa.PrivateKey{rfc, other}
	if _, err := x.RegisterSigningKeys([][32]byte{rfcPriv, otherPriv, {}}); err != nil {
		t.Fatal(err)
	}
	if _, err := x.RegisterKeys([][64]byte{rfcPub, otherPub}); err != nil {
		t.Fatal(err)
	}
	var votes []VoteMsg
	var idx []uint32
	for i := 0; i < 300; i++ {
		votes = append(votes, VoteMsg{ViewID: int64(i % 3), SequenceID: int64(i), Digest: Hash([]byte{byte(i)}),
			NodeID: []string{"Apple", "MS", "<n> ", ""}[i%4], MsgType: MsgType(1 + i%2)})
		idx = append(idx, uint32(i%2))
	}
	bad := len(votes)
	votes = append(votes, votes[0], votes[1])
	idx = append(idx, 2, 7) // an invalid key, an index past the set
	for _, format := range []SigFormat{SigRS, SigDER} {
		s, err := x.SealVotes(votes, idx, format)
		if err != nil {
			t.Fatal(err)
		}
		var pos uint64
		for i := 0; i < bad; i++ {
			msg := s.Message(i)
			if !s.OK[i] || s.Off[i] != pos {
				t.Fatalf("vote %d: ok %v, offset %d, want %d", i, s.OK[i], s.Off[i], pos)
			}
			pos += uint64(s.Len[i])
			var got signedVote
			if err := json.Unmarshal(msg, &got); err != nil || got.VoteMsg != votes[i] {
				t.Fatalf("vote %d: %s: %v", i, msg, err)
			}
			want, _ := json.Marshal(signedVote{votes[i], got.Signature})
			pre, _ := json.Marshal(votes[i])
			if !bytes.Equal(msg, want) || s.Digests[i] != sha256.Sum256(pre) {
				t.Errorf("vote %d: %s, json.Marshal gives %s", i, msg, want)
			}
			pub := &keys[idx[i]].PublicKey
			if format == SigDER {
				if !ecdsa.VerifyASN1(pub, s.Digests[i][:], got.Signature) {
					t.Errorf("vote %d: DER signature not accepted", i)
				}
			} else if len(got.Signature) != 64 || !ecdsa.Verify(pub, s.Digests[i][:],
				new(big.Int).SetBytes(got.Signature[:32]), new(big.Int).SetBytes(got.Signature[32:])) {
				t.Errorf("vote %d: r||s signature not accepted", i)
			}
		}
		for i := bad; i < len(votes); i++ {
			if s.OK[i] || s.Len[i] != 0 || s.Off[i] != pos || s.Message(i) != nil {
				t.Errorf("row %d: a bad key index sealed a message", i)
			}
		}
		if uint64(len(s.Wire)) != pos {
			t.Errorf("total %d, want %d", len(s.Wire), pos)
		}
	}
}

func TestSealedRepliesFeedFlushReplies(t *testing.T) {
	x := gpu(t)
	_, priv, pub := signKey(t, rfcKey)
	if _, err := x.RegisterSigningKeys([][32]byte{priv}); err != nil {
		t.Fatal(err)
	}
	if _, err := x.RegisterKeys([][64]byte{pub}); err != nil {
		t.Fatal(err)
	}
	reps := make([]ReplyMsg, 70)
	idx := make([]uint32, len(reps))
	for i := range reps {
		reps[i] = ReplyMsg{ViewID: int64(i % 3), Timestamp: int64(1000 + i), ClientID: "client<1>", NodeID: "Node",
			Result: "Executed"}
	}
	reps[5].Result = ""
	s, err := x.SealReplies(reps, idx, SigDER)
	if err != nil {
		t.Fatal(err)
	}
	back, sigs := make([]ReplyMsg, len(reps)), make([][]byte, len(reps))
	for i := range reps {
		var got struct {
			ReplyMsg
			Signature []byte `json:"signature"`
		}
		if err := json.Unmarshal(s.Message(i), &got); err != nil {
			t.Fatal(err)
		}
		back[i], sigs[i] = got.ReplyMsg, got.Signature
	}
	dg, ok, err := x.FlushRepliesASN1(back, sigs, idx)
	if err != nil {
		t.Fatal(err)
	}
	for i := range reps {
		if !ok[i] || dg[i] != s.Digests[i] || back[i] != reps[i] {
			t.Errorf("reply %d: accepted %v", i, ok[i])
		}
	}
}

func TestSealPrePreparesCarryTheClientsSignature(t *testing.T) {
	x := gpu(t)
	_, priv, _ := signKey(t, rfcKey)
	if _, err := x.RegisterSigningKeys([][32]byte{priv}); err != nil {
		t.Fatal(err)
	}
	req := &RequestMsg{Timestamp: 1668519246, ClientID: "client1", Operation: "printf", SequenceID: 7}
	pps := []PrePrepareMsg{{ViewID: 0, SequenceID: 7, Digest: "ab", RequestMsg: req},
		{ViewID: 0, SequenceID: 8, Digest: "cd", RequestMsg: req},
		{ViewID: 0, SequenceID: 9, Digest: "ef", RequestMsg: req},
		{ViewID: 1, SequenceID: 10, Digest: "", RequestMsg: nil}}
	reqSigs := [][]byte{[]byte("client signature bytes"), {}, nil, []byte("not read")}
	s, err := x.SealPrePrepares(pps, reqSigs, make([]uint32, len(pps)), SigRS)
	if err != nil {
		t.Fatal(err)
	}
	for i, p := range pps {
		var got signedPrePrepare
		if err := json.Unmarshal(s.Message(i), &got); err != nil {
			t.Fatal(err)
		}
		want := signedPrePrepare{ViewID: p.ViewID, SequenceID: p.SequenceID, Digest: p.Digest, Signature: got.Signature}
		if p.RequestMsg != nil {
			want.RequestMsg = &signedRequest{*p.RequestMsg, reqSigs[i]}
		}
		enc, _ := json.Marshal(want)
		pre, _ := json.Marshal(p)
		if !bytes.Equal(s.Message(i), enc) || s.Digests[i] != sha256.Sum256(pre) {
			t.Errorf("pre-prepare %d: %s, json.Marshal gives %s", i, s.Message(i), enc)
		}
	}
}
