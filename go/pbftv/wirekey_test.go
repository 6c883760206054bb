package pbftv

// Keys in SEC1 wire form: the library's decode (VerifyWireKeyBatch) against
// go1.19 elliptic.Unmarshal / UnmarshalCompressed on the golden keys, in the
// encodings elliptic.Marshal / MarshalCompressed write, with the wrong parity
// and with foreign prefix bytes.  The stdlib half needs no GPU; the library
// half is skipped where pbftv_open finds no gfx950 device.

import (
	"crypto/ecdsa"
	"crypto/elliptic"
	"math/big"
	"testing"
)

func TestWireKeysAgainstElliptic(t *testing.T) {
	var fx ecdsaFixtures
	load(t, "ecdsa.json", &fx)
	curve := elliptic.P256()
	p := curve.Params().P
	type wire struct {
		comp, flip, unc []byte // MarshalCompressed, the same with the other parity, Marshal
		pub, neg       *ecdsa.PublicKey
	}
	keys := make([]*wire, len(fx.Keys))
	for i, k := range fx.Keys {
		if !k.Valid {
			// the raw bytes as an uncompressed key: Unmarshal must refuse them
			raw := append([]byte{4}, append(unhex(t, k.X), unhex(t, k.Y)...)...)
			if x, _ := elliptic.Unmarshal(curve, raw); x != nil {
				t.Errorf("key %d: elliptic.Unmarshal accepts a key the fixture calls invalid", i)
			}
			continue
		}
		x, y := new(big.Int).SetBytes(unhex(t, k.X)), new(big.Int).SetBytes(unhex(t, k.Y))
		w := &wire{comp: elliptic.MarshalCompressed(curve, x, y), unc: elliptic.Marshal(curve, x, y),
			pub: &ecdsa.PublicKey{Curve: curve, X: x, Y: y}}
		w.flip = append([]byte{w.comp[0] ^ 1}, w.comp[1:]...)
		if gx, gy := elliptic.UnmarshalCompressed(curve, w.comp); gx == nil || gx.Cmp(x) != 0 || gy.Cmp(y) != 0 {
			t.Errorf("key %d: UnmarshalCompressed does not give the key back", i)
		}
		ny := new(big.Int).Sub(p, y)
		if gx, gy := elliptic.UnmarshalCompressed(curve, w.flip); gx == nil || gx.Cmp(x) != 0 || gy.Cmp(ny) != 0 {
			t.Errorf("key %d: the other prefix does not give (x, p - y)", i)
		}
		w.neg = &ecdsa.PublicKey{Curve: curve, X: x, Y: ny}
		for _, pre := range []byte{0, 1, 4, 5, 6, 7, 0xFF} {
			if gx, _ := elliptic.UnmarshalCompressed(curve, append([]byte{pre}, w.comp[1:]...)); gx != nil {
				t.Errorf("key %d: UnmarshalCompressed accepts prefix %02x", i, pre)
			}
		}
		for _, pre := range []byte{0, 2, 3, 6, 7} {
			if gx, _ := elliptic.Unmarshal(curve, append([]byte{pre}, w.unc[1:]...)); gx != nil {
				t.Errorf("key %d: Unmarshal accepts prefix %02x", i, pre)
			}
		}
		keys[i] = w
	}
	// every vector under a valid key, in four encodings: compressed, the other
	// parity, uncompressed, and uncompressed with a hybrid prefix (06)
	var hashes [][32]byte
	var sigs [][64]byte
	var comp, flip, unc, hyb []byte
	var want, wantFlip []bool
	for _, v := range fx.Vectors {
		if int(v.Key) >= len(keys) || keys[v.Key] == nil {
			continue
		}
		w := keys[v.Key]
		var h [32]byte
		var s [64]byte
		hb, r, sb := unhex(t, v.Hash), unhex(t, v.R), unhex(t, v.S)
		copy(h[:], hb)
		copy(s[:32], r)
		copy(s[32:], sb)
		hashes, sigs = append(hashes, h), append(sigs, s)
		comp, flip, unc = append(comp, w.comp...), append(flip, w.flip...), append(unc, w.unc...)
		hyb = append(hyb, append([]byte{6}, w.unc[1:]...)...)
		want = append(want, v.Expect)
		wantFlip = append(wantFlip, ecdsa.Verify(w.neg, hb, new(big.Int).SetBytes(r), new(big.Int).SetBytes(sb)))
	}
	x := gpu(t)
	check := func(name string, keys []byte, f KeyFormat, want []bool) {
		got, err := x.VerifyWireKeyBatch(hashes, sigs, keys, f)
		if err != nil {
			t.Fatal(err)
		}
		for i := range want {
			if got[i] != want[i] {
				t.Errorf("%s, signature %d: library %v, expected %v", name, i, got[i], want[i])
			}
		}
	}
	check("compressed", comp, KeySEC1Compressed, want)
	check("compressed, other parity", flip, KeySEC1Compressed, wantFlip)
	check("uncompressed", unc, KeySEC1Uncompressed, want)
	check("hybrid prefix", hyb, KeySEC1Uncompressed, make([]bool, len(want)))
}
