package pbftv

// Signing on the GPU against the standard library: every signature SignBatch,
// SignBatchASN1 and SignReplies return is accepted by go's crypto/ecdsa.Verify
// / VerifyASN1 under the matching public key and by this package's own
// verifies; the two P-256 / SHA-256 rows of RFC 6979 A.2.5 come out byte for
// byte; a bad key index signs nothing.  Skipped where pbftv_open finds no
// gfx950 device.
//
// NOTE: written without a Go toolchain at hand; it has not been compiled.

import (
	"crypto/ecdsa"
	"crypto/elliptic"
	"crypto/sha256"
	"encoding/hex"
	"math/big"
	"testing"
)

const rfcKey = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721"

var rfcRows = []struct{ msg, r, s string }{
	{"sample", "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716",
		"F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"},
	{"test", "F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367",
		"019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083"},
}

func signKey(t *testing.T, hexD string) (*ecdsa.PrivateKey, [32]byte, [64]byte) {
	t.Helper()
	d, _ := new(big.Int).SetString(hexD, 16)
	k := &ecdsa.PrivateKey{D: d}
	k.Curve = elliptic.P256()
	k.X, k.Y = k.Curve.ScalarBaseMult(d.Bytes())
	var priv [32]byte
	var pub [64]byte
	d.FillBytes(priv[:])
	k.X.FillBytes(pub[:32])
	k.Y.FillBytes(pub[32:])
	return k, priv, pub
}

func TestSignBatchAgainstStdlib(t *testing.T) {
	x := gpu(t)
	rfc, rfcPriv, rfcPub := signKey(t, rfcKey)
	other, otherPriv, otherPub := signKey(t, "0000000000000000000000000000000000000000000000000000000000000005")
	keys := []*ecdsa.PrivateKey{rfc, other}
	valid, err := x.RegisterSigningKeys([][32]byte{rfcPriv, otherPriv, {}})
	if err != nil || !valid[0] || !valid[1] || valid[2] {
		t.Fatalf("RegisterSigningKeys: %v %v", valid, err)
	}
	if _, err := x.RegisterKeys([][64]byte{rfcPub, otherPub}); err != nil {
		t.Fatal(err)
	}
	var hashes [][32]byte
	var idx []uint32
	for _, row := range rfcRows {
		hashes = append(hashes, sha256.Sum256([]byte(row.msg)))
		idx = append(idx, 0)
	}
	for i := 0; i < 300; i++ {
		hashes = append(hashes, sha256.Sum256([]byte{byte(i), byte(i >> 8)}))
		idx = append(idx, uint32(i%2))
	}
	bad := len(hashes)
	hashes = append(hashes, hashes[0], hashes[1])
	idx = append(idx, 2, 7) // an invalid key, an index past the set
	sigs, ok, err := x.SignBatch(hashes, idx)
	if err != nil {
		t.Fatal(err)
	}
	for i, row := range rfcRows {
		if hex.EncodeToString(sigs[i][:]) != hex.EncodeToString(unhex(t, row.r+row.s)) {
			t.Errorf("RFC 6979 row %q: got %x", row.msg, sigs[i])
		}
	}
	for i := 0; i < bad; i++ {
		r, s := new(big.Int).SetBytes(sigs[i][:32]), new(big.Int).SetBytes(sigs[i][32:])
		if !ok[i] || !ecdsa.Verify(&keys[idx[i]].PublicKey, hashes[i][:], r, s) {
			t.Errorf("signature %d: ok %v, not accepted by ecdsa.Verify", i, ok[i])
		}
	}
	for i := bad; i < len(hashes); i++ {
		if ok[i] || sigs[i] != [64]byte{} {
			t.Errorf("row %d: a bad key index signed", i)
		}
	}
	accepted, err := x.VerifySigs(hashes[:bad], sigs[:bad], idx[:bad])
	if err != nil {
		t.Fatal(err)
	}
	for i, a := range accepted {
		if !a {
			t.Errorf("signature %d: not accepted by VerifySigs", i)
		}
	}
	ders, err := x.SignBatchASN1(hashes, idx)
	if err != nil {
		t.Fatal(err)
	}
	for i := 0; i < bad; i++ {
		r, s := new(big.Int).SetBytes(sigs[i][:32]), new(big.Int).SetBytes(sigs[i][32:])
		if hex.EncodeToString(ders[i]) != hex.EncodeToString(encodeASN1(t, r, s)) ||
			!ecdsa.VerifyASN1(&keys[idx[i]].PublicKey, hashes[i][:], ders[i]) {
			t.Errorf("DER signature %d: %x", i, ders[i])
		}
	}
	if ders[bad] != nil || ders[bad+1] != nil {
		t.Errorf("a bad key index produced a DER signature")
	}
}

func TestSignRepliesFeedFlushReplies(t *testing.T) {
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
	dg, sigs, ok, err := x.SignReplies(reps, idx)
	if err != nil {
		t.Fatal(err)
	}
	fdg, fok, err := x.FlushReplies(reps, sigs, idx)
	if err != nil {
		t.Fatal(err)
	}
	for i := range reps {
		if !ok[i] || !fok[i] || dg[i] != fdg[i] {
			t.Errorf("reply %d: signed %v, accepted %v, digests equal %v", i, ok[i], fok[i], dg[i] == fdg[i])
		}
	}
	dg2, ders, err := x.SignRepliesASN1(reps, idx)
	if err != nil {
		t.Fatal(err)
	}
	_, dok, err := x.FlushRepliesASN1(reps, ders, idx)
	if err != nil {
		t.Fatal(err)
	}
	for i := range reps {
		if !dok[i] || dg2[i] != dg[i] {
			t.Errorf("reply %d: DER signature not accepted", i)
		}
	}
}
