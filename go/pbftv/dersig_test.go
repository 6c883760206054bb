package pbftv

// Signatures as ASN.1 DER: the library's parse on the GPU (VerifySigsASN1,
// VerifyWireKeyBatchASN1) against go1.19 crypto/ecdsa.VerifyASN1 on the
// golden vectors -- encoded the way ecdsa.SignASN1 does, then broken the ways a parser can be
// fooled: a trailing byte inside and after the sequence, a long-form length,
// a padded or negative integer, a truncation, an empty signature.  The stdlib
// half needs no GPU; the library half is skipped where pbftv_open finds no
// gfx950 device.
//
// NOTE: written without a Go toolchain at hand; it has not been compiled.

import (
	"crypto/ecdsa"
	"crypto/elliptic"
	"encoding/asn1"
	"math/big"
	"testing"
)

// encodeASN1 gives the bytes ecdsa.SignASN1 returns for (r, s): the DER of
// SEQUENCE { INTEGER r, INTEGER s } (the standard library only; the module has
// no dependencies).
func encodeASN1(t *testing.T, r, s *big.Int) []byte {
	t.Helper()
	out, err := asn1.Marshal(struct{ R, S *big.Int }{r, s})
	if err != nil {
		t.Fatal(err)
	}
	return out
}

// mangle returns the variants of a valid encoding e that VerifyASN1 must refuse
// (and, first, e itself).
func mangle(e []byte) [][]byte {
	cat := func(parts ...[]byte) []byte {
		var out []byte
		for _, p := range parts {
			out = append(out, p...)
		}
		return out
	}
	lr := int(e[3])
	r, s := e[4:4+lr], e[6+lr:]
	intTLV := func(v []byte) []byte { return cat([]byte{2, byte(len(v))}, v) }
	seq := func(body []byte) []byte { return cat([]byte{0x30, byte(len(body))}, body) }
	return [][]byte{
		e,
		cat(e, []byte{0}),                                   // a byte after the sequence
		cat([]byte{0x30, e[1] + 1}, e[2:], []byte{0}),       // a byte inside it, after s
		cat([]byte{0x30, 0x81, e[1]}, e[2:]),                // long form for a short length
		cat([]byte{0x30, 0x82, 0, e[1]}, e[2:]),             // ... with a leading zero
		seq(cat(intTLV(cat([]byte{0}, r)), intTLV(s))),      // r padded with a redundant 00
		seq(cat(intTLV(cat([]byte{0x80}, r[1:])), intTLV(s))), // r negative
		seq(cat(intTLV(r), intTLV(nil))),                    // s of length 0
		cat([]byte{0x31}, e[1:]),                            // SET, not SEQUENCE
		e[:len(e)-1],                                        // truncated
		e[:2],
		{},
	}
}

func TestASN1SignaturesAgainstVerifyASN1(t *testing.T) {
	var fx ecdsaFixtures
	load(t, "ecdsa.json", &fx)
	curve := elliptic.P256()
	pubs := make([]*ecdsa.PublicKey, len(fx.Keys))
	var regKeys [][64]byte
	for i, k := range fx.Keys {
		var xy [64]byte
		copy(xy[:32], unhex(t, k.X))
		copy(xy[32:], unhex(t, k.Y))
		regKeys = append(regKeys, xy)
		if k.Valid {
			pubs[i] = &ecdsa.PublicKey{Curve: curve, X: new(big.Int).SetBytes(xy[:32]), Y: new(big.Int).SetBytes(xy[32:])}
		}
	}
	var hashes [][32]byte
	var ders [][]byte
	var keyIdx []uint32
	var unc []byte
	var want []bool
	accepted, refused := 0, 0
	for _, v := range fx.Vectors {
		if int(v.Key) >= len(pubs) || pubs[v.Key] == nil {
			continue
		}
		hb := unhex(t, v.Hash)
		e := encodeASN1(t, new(big.Int).SetBytes(unhex(t, v.R)), new(big.Int).SetBytes(unhex(t, v.S)))
		if ecdsa.VerifyASN1(pubs[v.Key], hb, e) != v.Expect {
			t.Errorf("VerifyASN1 disagrees with the fixture on its own encoding")
		}
		vars := [][]byte{e}
		if v.Expect {
			vars = mangle(e)
		}
		for j, d := range vars {
			var h [32]byte
			copy(h[:], hb)
			ok := ecdsa.VerifyASN1(pubs[v.Key], hb, d)
			if j > 0 && ok {
				t.Errorf("VerifyASN1 accepts the mangled encoding %x", d)
			}
			hashes, ders, keyIdx, want = append(hashes, h), append(ders, d), append(keyIdx, v.Key), append(want, ok)
			unc = append(unc, elliptic.Marshal(curve, pubs[v.Key].X, pubs[v.Key].Y)...)
			if ok {
				accepted++
			} else {
				refused++
			}
		}
	}
	if accepted == 0 || refused == 0 {
		t.Fatalf("the vectors must hold both outcomes: %d accepted, %d refused", accepted, refused)
	}
	x := gpu(t)
	if _, err := x.RegisterKeys(regKeys); err != nil {
		t.Fatal(err)
	}
	compare := func(name string, got []bool, err error) {
		if err != nil {
			t.Fatal(err)
		}
		for i := range want {
			if got[i] != want[i] {
				t.Errorf("%s, signature %d (%x): library %v, VerifyASN1 %v", name, i, ders[i], got[i], want[i])
			}
		}
	}
	got, err := x.VerifySigsASN1(hashes, ders, keyIdx) // small: host parse, latency path
	compare("registered", got, err)
	if err := x.SetLatencyPathMax(0); err != nil { // the device normaliser
		t.Fatal(err)
	}
	got, err = x.VerifySigsASN1(hashes, ders, keyIdx)
	compare("registered, lane path", got, err)
	if err := x.SetLatencyPathMax(2048); err != nil {
		t.Fatal(err)
	}
	got, err = x.VerifyWireKeyBatchASN1(hashes, ders, unc, KeySEC1Uncompressed)
	compare("carried keys", got, err)
}
