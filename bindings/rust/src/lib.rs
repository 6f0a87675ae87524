//! Safe layer over libkmx that keeps the `kmers` crate's own surface.
//!
//! A GPU is a drop-in only at batch granularity, so every type here offers the crate's scalar interface (one k-mer
//! per call = a one-element batch: the correctness path, bit-identical to the CPU implementation) next to a batch
//! form (the throughput path).  Reference lines (`kmers` @ COMBINE-lab) are cited per item.
//!
//! * [`HipEncoder`]             — `impl Encoding<P, B>` for every `utils::Data` word type P = u8 .. u128 (src/encoding/mod.rs:14-23,
//!                                src/encoding/naive.rs:112-115, src/utils.rs:4-24) and every `Naive` map (+ Xor10 = `Naive::ACTG`)
//! * [`HipCanonicalKmerBatch`]  — `CanonicalKmerIterator` over many reads (src/naive_impl/canonical_kmer_iterator.rs:42-116);
//!                                [`HipCanonicalKmerIter`] walks one read of it with the crate's own `inc` / `get` / `exhausted`
//! * [`canonical_sum`]          — the consumer shape of benches/simple_benchmark.rs:14-22 on device-resident reads
//! * [`HipSeqVector`]           — `SeqVector` (src/naive_impl/seq_vector.rs) with the words on the device
//! * [`HipComm`]                — the RCCL exchange of the optional bucket histogram (no counterpart: the crate is single-process)
pub mod ffi;

use ffi::*;
use kmers::encoding::{Encoding, Naive};
use kmers::utils::Data;
use std::os::raw::c_void;
use std::ptr;

/// Error = a libkmx status code (`KMX_E_*`) with its text.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct KmxError {
    pub status: i32,
    pub message: String,
}

fn check(ctx: *const kmx_ctx, status: i32) -> Result<(), KmxError> {
    if status == KMX_OK {
        return Ok(());
    }
    let mut message = unsafe { std::ffi::CStr::from_ptr(kmx_strerror(status)) }.to_string_lossy().into_owned();
    if status == KMX_E_HIP && !ctx.is_null() {
        message.push_str(" -- ");
        message.push_str(&unsafe { std::ffi::CStr::from_ptr(kmx_last_error(ctx)) }.to_string_lossy());
    }
    Err(KmxError { status, message })
}

/// One `kmx_ctx`: a device, a HIP stream, scratch.  Single-threaded like the ABI says (one per host thread / GPU).
pub struct HipContext(*mut kmx_ctx);

impl HipContext {
    pub fn new(device: i32) -> Result<Self, KmxError> {
        let mut p = ptr::null_mut();
        check(ptr::null(), unsafe { kmx_ctx_create(device, &mut p) })?;
        Ok(Self(p))
    }
    pub fn synchronize(&self) -> Result<(), KmxError> {
        check(self.0, unsafe { kmx_ctx_synchronize(self.0) })
    }
    pub fn raw(&self) -> *mut kmx_ctx {
        self.0
    }
    fn ck(&self, status: i32) -> Result<(), KmxError> {
        check(self.0, status)
    }
    /// `n` bytes of device memory, freed on drop
    pub fn alloc(&self, n: usize) -> Result<DeviceBuf<'_>, KmxError> {
        let mut p = ptr::null_mut();
        self.ck(unsafe { kmx_malloc(self.0, n, &mut p) })?;
        Ok(DeviceBuf { ctx: self, ptr: p, len: n })
    }
    pub fn upload(&self, host: &[u8]) -> Result<DeviceBuf<'_>, KmxError> {
        let b = self.alloc(host.len())?;
        self.ck(unsafe { kmx_memcpy_h2d(self.0, b.ptr, host.as_ptr() as *const c_void, host.len()) })?;
        Ok(b)
    }
}

impl Drop for HipContext {
    fn drop(&mut self) {
        unsafe { kmx_ctx_destroy(self.0) }
    }
}

/// Device allocation owned by a context.
pub struct DeviceBuf<'c> {
    ctx: &'c HipContext,
    ptr: *mut c_void,
    len: usize,
}

impl<'c> DeviceBuf<'c> {
    pub fn as_ptr<T>(&self) -> *const T {
        self.ptr as *const T
    }
    pub fn as_mut_ptr<T>(&self) -> *mut T {
        self.ptr as *mut T
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    pub fn download<T: Copy + Default>(&self, n: usize) -> Result<Vec<T>, KmxError> {
        let mut v = vec![T::default(); n];
        assert!(n * std::mem::size_of::<T>() <= self.len);
        self.ctx.ck(unsafe { kmx_memcpy_d2h(self.ctx.0, v.as_mut_ptr() as *mut c_void, self.ptr, n * std::mem::size_of::<T>()) })?;
        Ok(v)
    }
}

impl<'c> Drop for DeviceBuf<'c> {
    fn drop(&mut self) {
        unsafe {
            kmx_free(self.ctx.0, self.ptr);
        }
    }
}

// ------------------------------------------------------------------------------------------------ Encoding

/// Drop-in for `impl Encoding<u64, B> for Naive` (src/encoding/naive.rs:112-154): the scalar trait methods run a
/// one-element batch; `encode_batch` / `decode_batch` / `rev_comp_batch` are the throughput forms.
/// `Xor10` (src/encoding/xor10.rs) is the same map as `Naive::ACTG`, so `HipEncoder { enc: Naive::ACTG, .. }` covers it
/// (its B == 1 `rev_comp`, xor10.rs:75-85, is not a reverse complement in the crate and is deliberately not reproduced).
pub struct HipEncoder<'c> {
    pub ctx: &'c HipContext,
    pub enc: Naive,
}

impl<'c> HipEncoder<'c> {
    pub fn new(ctx: &'c HipContext, enc: Naive) -> Self {
        Self { ctx, enc }
    }

    /// the little-endian byte image of a `[P; B]` slice (what the `_p` calls of the C ABI take: bit_field puts flat bit i into
    /// word i / BITS, bit i % BITS, so that image is the same flat bit string for every P -- include/kmx.h)
    fn bytes_of<P: Data>(words: &[P]) -> &[u8] {
        unsafe { std::slice::from_raw_parts(words.as_ptr() as *const u8, std::mem::size_of_val(words)) }
    }

    /// `seqs`: n sequences of `seq_len` bytes, contiguous -> n * B words of P.  Panics where the crate panics
    /// (`bit_field` index out of bounds when `2 * seq_len > P::BITS * B`, naive.rs:120).
    pub fn encode_batch<P: Data + Default, const B: usize>(&self, seqs: &[u8], seq_len: usize) -> Result<Vec<P>, KmxError> {
        let n = if seq_len == 0 { 0 } else { seqs.len() / seq_len };
        let wb = std::mem::size_of::<P>();
        let d_s = self.ctx.upload(seqs)?;
        let d_w = self.ctx.alloc(wb * B * n.max(1))?;
        let st = unsafe { kmx_encode_kmers_p(self.ctx.0, d_s.as_ptr(), n as u64, seq_len as u32, self.enc as u8, 8 * wb as u32, B as u32, d_w.as_mut_ptr()) };
        assert_ne!(st, KMX_E_TOO_LONG, "index out of bounds: the sequence is longer than the k-mer storage");
        self.ctx.ck(st)?;
        d_w.download::<P>(B * n)
    }

    /// `Encoding::decode` per k-mer: ALL `P::BITS * B / 2` letters each (naive.rs:126-136)
    pub fn decode_batch<P: Data, const B: usize>(&self, words: &[P]) -> Result<Vec<u8>, KmxError> {
        let n = words.len() / B;
        let wb = std::mem::size_of::<P>();
        let letters = 4 * wb * B;
        let d_w = self.ctx.upload(Self::bytes_of(words))?;
        let d_s = self.ctx.alloc(letters * n.max(1))?;
        self.ctx.ck(unsafe { kmx_encoding_decode_p(self.ctx.0, d_w.as_ptr(), n as u64, self.enc as u8, 8 * wb as u32, B as u32, d_s.as_mut_ptr()) })?;
        d_s.download::<u8>(letters * n)
    }

    /// `Encoding::rev_comp::<K>` per k-mer (naive.rs:138-154): base i = complement(base K-1-i) for i < K, bits >= 2K unchanged
    pub fn rev_comp_batch<P: Data + Default, const B: usize>(&self, words: &[P], big_k: usize) -> Result<Vec<P>, KmxError> {
        let n = words.len() / B;
        let wb = std::mem::size_of::<P>();
        let d_in = self.ctx.upload(Self::bytes_of(words))?;
        let d_out = self.ctx.alloc((wb * words.len()).max(1))?;
        let st = unsafe { kmx_encoding_rev_comp_p(self.ctx.0, d_in.as_ptr(), n as u64, big_k as u32, self.enc as u8, 8 * wb as u32, B as u32, d_out.as_mut_ptr()) };
        assert_ne!(st, KMX_E_K_RANGE, "attempt to subtract with overflow"); // K == 1 in the crate (naive.rs:140,150)
        self.ctx.ck(st)?;
        d_out.download::<P>(words.len())
    }
}

/// `impl<P, const B: usize> Encoding<P, B> for Naive where P: utils::Data` (src/encoding/naive.rs:112-115), on the device:
/// P = u8, u16, u32, u64, u128 (src/utils.rs:24).
impl<'c, P: Data + Default, const B: usize> Encoding<P, B> for HipEncoder<'c> {
    fn encode(&self, seq: &[u8]) -> [P; B] {
        let v = self.encode_batch::<P, B>(seq, seq.len().max(1)).expect("Encoding::encode");
        let mut out = [P::default(); B];
        if !seq.is_empty() {
            out.copy_from_slice(&v[..B]);
        }
        out
    }

    fn decode(&self, array: [P; B]) -> Vec<u8> {
        self.decode_batch::<P, B>(&array).expect("Encoding::decode")
    }

    fn rev_comp<const K: usize>(&self, array: [P; B]) -> [P; B] {
        let v = self.rev_comp_batch::<P, B>(&array, K).expect("Encoding::rev_comp");
        let mut out = [P::default(); B];
        out.copy_from_slice(&v[..B]);
        out
    }
}

// ------------------------------------------------------------------------------------------------ CanonicalKmerIterator

/// Batch form of `for km in CanonicalKmerIterator::from_u8_slice(read, k)` over many reads
/// (src/naive_impl/canonical_kmer_iterator.rs:72-116): holds, per window slot, what the iterator's `get()` would show.
pub struct HipCanonicalKmerBatch {
    pub fw: Vec<u64>,
    pub rc: Vec<u64>,
    pub flags: Vec<u8>,
    pub windows_per_read: usize,
}

impl HipCanonicalKmerBatch {
    /// `reads`: n_reads x read_len ASCII bytes, contiguous.  k in 1..=31 (the crate's MASK_TABLE[32] == 0, kmer.rs:617).
    pub fn scan(ctx: &HipContext, reads: &[u8], read_len: usize, k: u8) -> Result<Self, KmxError> {
        let n_reads = if read_len == 0 { 0 } else { reads.len() / read_len };
        let w = (read_len + 1).saturating_sub(k as usize);
        let total = n_reads * w;
        let d_b = ctx.upload(reads)?;
        let (d_fw, d_rc, d_fl) = (ctx.alloc(8 * total.max(1))?, ctx.alloc(8 * total.max(1))?, ctx.alloc(total.max(1))?);
        let r = kmx_reads { d_bases: d_b.as_ptr(), n_reads: n_reads as u64, read_len: read_len as u32, d_offsets: ptr::null() };
        ctx.ck(unsafe { kmx_canonical_windows(ctx.0, &r, ptr::null(), k as u32, d_fw.as_mut_ptr(), d_rc.as_mut_ptr(), ptr::null_mut(), d_fl.as_mut_ptr()) })?;
        Ok(Self { fw: d_fw.download(total)?, rc: d_rc.download(total)?, flags: d_fl.download(total)?, windows_per_read: w })
    }

    /// (read, pos, fw word, rc word) for every window the crate's iterator yields, in its order;
    /// `CanonicalKmer::get_canonical_word()` (canonical_kmer.rs:113-119) is `if fw < rc { fw } else { rc }`.
    pub fn iter(&self) -> impl Iterator<Item = (usize, i32, u64, u64)> + '_ {
        let w = self.windows_per_read.max(1);
        self.flags.iter().enumerate().filter(|(_, f)| **f & KMX_WIN_VALID != 0).map(move |(i, _)| (i / w, (i % w) as i32, self.fw[i], self.rc[i]))
    }
}

/// What `CanonicalKmerIterator::get()` shows (canonical_kmer_iterator.rs:13-16,113-116): the k-mer pair and its offset on the read.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct HipCanonicalKmerPos {
    pub fw: u64,
    pub rc: u64,
    pub pos: i32,
}

impl HipCanonicalKmerPos {
    /// `CanonicalKmer::get_canonical_word()` (canonical_kmer.rs:113-119)
    pub fn canonical_word(&self) -> u64 {
        if self.fw < self.rc { self.fw } else { self.rc }
    }
}

/// One read of a [`HipCanonicalKmerBatch`] behind the crate's iterator protocol
/// (canonical_kmer_iterator.rs:89-116): `from_u8_slice` positions on the first valid k-mer, `inc()` moves to the next and
/// returns whether there is one, `exhausted()` tells when there is none, `get()` shows the current pair -- so a loop written
/// as `while !it.exhausted() { use(it.get()); it.inc(); }` against the crate runs unchanged over a scanned batch.
pub struct HipCanonicalKmerIter<'b> {
    batch: &'b HipCanonicalKmerBatch,
    base: usize,      // first window slot of the read
    slot: usize,      // current window (valid only while !invalid)
    invalid: bool,
}

impl<'b> HipCanonicalKmerIter<'b> {
    fn seek(&mut self, from: usize) {
        let w = self.batch.windows_per_read;
        let mut i = from;
        while i < w && self.batch.flags[self.base + i] & KMX_WIN_VALID == 0 {
            i += 1;
        }
        self.invalid = i >= w;
        self.slot = i;
    }
    /// `exhausted()` (canonical_kmer_iterator.rs:89-92)
    pub fn exhausted(&self) -> bool {
        self.invalid
    }
    /// `inc()` (canonical_kmer_iterator.rs:94-102)
    pub fn inc(&mut self) -> bool {
        if !self.invalid {
            let next = self.slot + 1;
            self.seek(next);
        }
        !self.invalid
    }
    /// `inc_by(count)` (canonical_kmer_iterator.rs:104-112)
    pub fn inc_by(&mut self, mut count: usize) -> bool {
        let mut v = !self.invalid;
        while count > 0 && v {
            v = self.inc();
            count -= 1;
        }
        v
    }
    /// `get()` (canonical_kmer_iterator.rs:113-116); like the crate's, meaningful while `!exhausted()`
    pub fn get(&self) -> HipCanonicalKmerPos {
        let i = self.base + self.slot.min(self.batch.windows_per_read.saturating_sub(1));
        HipCanonicalKmerPos { fw: self.batch.fw[i], rc: self.batch.rc[i], pos: self.slot as i32 }
    }
}

impl HipCanonicalKmerBatch {
    /// the iterator of read `read` (`CanonicalKmerIterator::from_u8_slice(read_bytes, k)`, canonical_kmer_iterator.rs:72-83)
    pub fn read_iter(&self, read: usize) -> HipCanonicalKmerIter<'_> {
        let mut it = HipCanonicalKmerIter { batch: self, base: read * self.windows_per_read, slot: 0, invalid: self.windows_per_read == 0 };
        if !it.invalid {
            it.seek(0);
        }
        it
    }
}

/// The consumer shape of benches/simple_benchmark.rs:14-22 (`.sum()` over the words of all windows) on device-resident
/// reads: count, wrapping sum of canonical words, xor of `hash_one(LexHasherState::new(k), ..)`, wrapping sum of fw words.
pub fn canonical_sum(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8) -> Result<kmx_summary, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    // (the summary straight into host memory: one kernel launch for clean reads of up to 256 bases, no device allocation, no copy)
    let mut out = std::mem::MaybeUninit::<kmx_summary>::zeroed();
    ctx.ck(unsafe { kmx_canonical_reduce_host(ctx.0, &r, k as u32, KMX_HASH_LEX, k as u32, KMX_REDUCE_SUM_FW, out.as_mut_ptr()) })?;
    Ok(unsafe { out.assume_init() })
}

/// `hash_one(&state, kmer)` for a batch of k-mer words with one of std's `BuildHasher`s (src/naive_impl/hash.rs:10-20): std's
/// `DefaultHasher` is SipHash-1-3 and `impl Hash for Kmer` feeds it one `write_u64(data)` (hash.rs:4-8).  `keys` = (0, 0) for
/// `DefaultHasher::new()` / `BuildHasherDefault<DefaultHasher>`; a `RandomState`'s keys are private to std, so a caller who wants
/// device hashes equal to host hashes builds its hasher from keys it knows (`SipHasher13::new_with_keys` semantics).
pub fn hash_words_sip13(ctx: &HipContext, words: &[u64], keys: (u64, u64)) -> Result<Vec<u64>, KmxError> {
    // (the device takes the words as they lie in memory: little-endian u64, what `write_u64` hashes on every target this library runs beside)
    let bytes = unsafe { std::slice::from_raw_parts(words.as_ptr() as *const u8, words.len() * 8) };
    let d_in = ctx.upload(bytes)?;
    let d_out = ctx.alloc(words.len() * 8)?;
    ctx.ck(unsafe { kmx_hash_words_sip13(ctx.0, d_in.as_ptr::<u64>(), words.len() as u64, keys.0, keys.1, d_out.as_mut_ptr::<u64>()) })?;
    d_out.download::<u64>(words.len())
}

/// `SeqVector::from(read).iter_minimizers(k, w, LexHasherState::new(lex_hasher_k))` (seq_vector.rs:73-80, minimizers.rs:39-141)
/// for every read of a uniform batch already on the device, without building the `SeqVector`s: `(word, pos)` of k-mer `i` of read
/// `r` at index `r * (read_len - k + 1) + i`.  A byte outside ACGTacgt is the panic of `Kmer::from` (kmer.rs:45-60): `Err` with
/// `KMX_E_INVALID_BASE`.
pub fn minimizers_of_reads(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, w: u8, lex_hasher_k: u8)
                           -> Result<Vec<(u64, u32)>, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(read_len >= k as u32, "SeqVecMinimizerIter::new: assertion failed: sv.len() >= k");
    let n = (n_reads * (read_len - k as u32 + 1) as u64) as usize;
    let d_word = ctx.alloc(n * 8)?;
    let d_pos = ctx.alloc(n * 4)?;
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut first_bad = u64::MAX;
    ctx.ck(unsafe { kmx_minimizers(ctx.0, &r, ptr::null(), k as u32, w as u32, KMX_HASH_LEX, lex_hasher_k as u32, d_word.as_mut_ptr::<u64>(),
                                   d_pos.as_mut_ptr::<u32>(), &mut first_bad) })?;
    let (a, b) = (d_word.download::<u64>(n)?, d_pos.download::<u32>(n)?);
    Ok(a.into_iter().zip(b).collect())
}

/// The canonical k-mer scan of a uniform batch already on the device with std's `DefaultHasher` (`keys = (0, 0)`) or a
/// `RandomState` (its two keys) folded in: `xor_hash` = xor of SipHash-1-3(keys; canonical word) (`kmx_canonical_reduce_sip13`).
pub fn canonical_reduce_sip13(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, keys: (u64, u64), flags: u32)
                              -> Result<kmx_summary, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    let d_out = ctx.alloc(std::mem::size_of::<kmx_summary>())?;
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_canonical_reduce_sip13(ctx.0, &r, k as u32, keys.0, keys.1, flags, d_out.as_mut_ptr()) })?;
    Ok(d_out.download::<kmx_summary>(1)?[0])
}

/// Bucket counts of SipHash-1-3(keys; canonical word) over a uniform batch already on the device (`kmx_histogram_sip13`,
/// 2^log2_buckets counters, the BUILD-DEFINED bucket function of `kmx_histogram`)
pub fn histogram_sip13(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, keys: (u64, u64), log2_buckets: u32)
                       -> Result<Vec<u64>, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    let nb = 1usize << log2_buckets.min(30);
    let d_counts = ctx.alloc(8 * nb)?;
    ctx.ck(unsafe { kmx_memset(ctx.0, d_counts.as_mut_ptr(), 0, d_counts.len()) })?;
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_histogram_sip13(ctx.0, &r, k as u32, keys.0, keys.1, log2_buckets, d_counts.as_mut_ptr::<u64>()) })?;
    d_counts.download::<u64>(nb)
}

/// Exact count of the canonical k-mers of a uniform batch already on the device (`kmx_count_canonical`): the distinct
/// canonical words in ascending order with how many windows yield each.  `d_kmers` / `d_counts` hold at least `max_distinct`
/// u64 each; Err(KMX_E_NOMEM) if the batch has more distinct k-mers (or its working set is above the work buffer's cap).
pub fn count_canonical(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, d_kmers: &DeviceBuf<'_>,
                       d_counts: &DeviceBuf<'_>, max_distinct: u64) -> Result<u64, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(max_distinct as u128 * 8 <= d_kmers.len().min(d_counts.len()) as u128, "outputs shorter than max_distinct");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut n_distinct = 0u64;
    ctx.ck(unsafe { kmx_count_canonical(ctx.0, &r, k as u32, d_kmers.as_mut_ptr::<u64>(), d_counts.as_mut_ptr::<u64>(), max_distinct,
                                        &mut n_distinct) })?;
    Ok(n_distinct)
}

/// The same count for two-word k-mers, k in 33..=64 (`kmx_count_canonical2`): `d_kmers2` holds at least `2 * max_distinct` u64 --
/// entry i is (low word, high word), ascending as a 2k-bit unsigned integer (high word first) -- and `d_counts` at least
/// `max_distinct`; Err(KMX_E_NOMEM) if the batch has more distinct k-mers (or its working set is above the work buffer's cap).
pub fn count_canonical2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, d_kmers2: &DeviceBuf<'_>,
                        d_counts: &DeviceBuf<'_>, max_distinct: u64) -> Result<u64, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(max_distinct as u128 * 16 <= d_kmers2.len() as u128 && max_distinct as u128 * 8 <= d_counts.len() as u128,
            "outputs shorter than max_distinct");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut n_distinct = 0u64;
    ctx.ck(unsafe { kmx_count_canonical2(ctx.0, &r, k as u32, d_kmers2.as_mut_ptr::<u64>(), d_counts.as_mut_ptr::<u64>(), max_distinct,
                                         &mut n_distinct) })?;
    Ok(n_distinct)
}

/// Union of two tables of `count_canonical2` (`kmx_count_merge2`): `a` and `b` are (keys, counts, entries); equal k-mers are
/// merged and their counts added.  `d_kmers2_out` holds at least `2 * max_out` u64, `d_counts_out` at least `max_out`.
pub fn count_merge2(ctx: &HipContext, a: (&DeviceBuf<'_>, &DeviceBuf<'_>, u64), b: (&DeviceBuf<'_>, &DeviceBuf<'_>, u64),
                    d_kmers2_out: &DeviceBuf<'_>, d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    for (keys, counts, n) in [a, b] {
        assert!(n as u128 * 16 <= keys.len() as u128 && n as u128 * 8 <= counts.len() as u128, "table shorter than its entry count");
    }
    assert!(max_out as u128 * 16 <= d_kmers2_out.len() as u128 && max_out as u128 * 8 <= d_counts_out.len() as u128,
            "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_merge2(ctx.0, a.0.as_ptr::<u64>(), a.1.as_ptr::<u64>(), a.2, b.0.as_ptr::<u64>(), b.1.as_ptr::<u64>(), b.2,
                                     d_kmers2_out.as_mut_ptr::<u64>(), d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

// ------------------------------------------------------------------------------------------------ the counting sketch

/// A counting sketch on the device (`kmx_sketch_*`, include/kmx.h "the counting sketch"): `64 << log2_blocks` saturating byte
/// cells, zero when new and accumulated into; a key's four cells lie in one 64-byte block chosen by its hash under `seed`.
pub struct Sketch<'c> {
    pub cells: DeviceBuf<'c>,
    pub log2_blocks: u32,
    pub seed: u64,
}

/// A zeroed sketch of `2^log2_blocks` blocks (`log2_blocks <= 32`).
pub fn sketch_new(ctx: &HipContext, log2_blocks: u32, seed: u64) -> Result<Sketch<'_>, KmxError> {
    assert!(log2_blocks <= 32, "log2_blocks above 32");
    let cells = ctx.alloc(64usize << log2_blocks)?;
    ctx.ck(unsafe { kmx_memset(ctx.0, cells.as_mut_ptr(), 0, cells.len()) })?;
    Ok(Sketch { cells, log2_blocks, seed })
}

fn sketch_reads(d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32) -> kmx_reads {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() }
}

/// Weight 1 for every valid window of a uniform batch already on the device (`kmx_sketch_add`, k in 1..=31).
pub fn sketch_add(ctx: &HipContext, sketch: &Sketch<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8) -> Result<(), KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    ctx.ck(unsafe { kmx_sketch_add(ctx.0, &r, k as u32, sketch.cells.as_mut_ptr::<u8>(), sketch.log2_blocks, sketch.seed) })
}

/// The same for two-word k-mers, k in 33..=64 (`kmx_sketch_add2`).
pub fn sketch_add2(ctx: &HipContext, sketch: &Sketch<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8) -> Result<(), KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    ctx.ck(unsafe { kmx_sketch_add2(ctx.0, &r, k as u32, sketch.cells.as_mut_ptr::<u8>(), sketch.log2_blocks, sketch.seed) })
}

/// `n` one-word keys as they are, each with its u64 weight (clipped to 255) or 1 (`kmx_sketch_add_words`): a table with its counts,
/// or the canonical words of a windows call.
pub fn sketch_add_words(ctx: &HipContext, sketch: &Sketch<'_>, d_words: &DeviceBuf<'_>, d_weights: Option<&DeviceBuf<'_>>, n: u64)
                        -> Result<(), KmxError> {
    assert!(n as u128 * 8 <= d_words.len() as u128 && d_weights.map_or(true, |w| n as u128 * 8 <= w.len() as u128), "keys or weights shorter than n");
    let w = d_weights.map_or(ptr::null(), |w| w.as_ptr::<u64>());
    ctx.ck(unsafe { kmx_sketch_add_words(ctx.0, d_words.as_ptr::<u64>(), w, n, sketch.cells.as_mut_ptr::<u8>(), sketch.log2_blocks, sketch.seed) })
}

/// The same for two-word keys, (low, high) pairs (`kmx_sketch_add_words2`).
pub fn sketch_add_words2(ctx: &HipContext, sketch: &Sketch<'_>, d_words2: &DeviceBuf<'_>, d_weights: Option<&DeviceBuf<'_>>, n: u64)
                         -> Result<(), KmxError> {
    assert!(n as u128 * 16 <= d_words2.len() as u128 && d_weights.map_or(true, |w| n as u128 * 8 <= w.len() as u128), "keys or weights shorter than n");
    let w = d_weights.map_or(ptr::null(), |w| w.as_ptr::<u64>());
    ctx.ck(unsafe { kmx_sketch_add_words2(ctx.0, d_words2.as_ptr::<u64>(), w, n, sketch.cells.as_mut_ptr::<u8>(), sketch.log2_blocks, sketch.seed) })
}

/// The estimate of `n` one-word keys (`kmx_sketch_lookup`): never below min(255, the key's true total).
pub fn sketch_lookup(ctx: &HipContext, sketch: &Sketch<'_>, d_words: &DeviceBuf<'_>, n: u64) -> Result<Vec<u8>, KmxError> {
    assert!(n as u128 * 8 <= d_words.len() as u128, "keys shorter than n");
    let d_est = ctx.alloc(n as usize + 1)?;
    ctx.ck(unsafe { kmx_sketch_lookup(ctx.0, d_words.as_ptr::<u64>(), n, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed,
                                      d_est.as_mut_ptr::<u8>()) })?;
    d_est.download::<u8>(n as usize)
}

/// The same for two-word keys (`kmx_sketch_lookup2`).
pub fn sketch_lookup2(ctx: &HipContext, sketch: &Sketch<'_>, d_words2: &DeviceBuf<'_>, n: u64) -> Result<Vec<u8>, KmxError> {
    assert!(n as u128 * 16 <= d_words2.len() as u128, "keys shorter than n");
    let d_est = ctx.alloc(n as usize + 1)?;
    ctx.ck(unsafe { kmx_sketch_lookup2(ctx.0, d_words2.as_ptr::<u64>(), n, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed,
                                       d_est.as_mut_ptr::<u8>()) })?;
    d_est.download::<u8>(n as usize)
}

/// One estimate per window of a uniform batch, read r at `r * (read_len - k + 1)`; 0 for a window with an invalid byte
/// (`kmx_sketch_lookup_reads`, k in 1..=31).
pub fn sketch_lookup_reads(ctx: &HipContext, sketch: &Sketch<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8)
                           -> Result<Vec<u8>, KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    let n = n_reads as usize * (read_len as usize + 1).saturating_sub(k as usize);
    let d_est = ctx.alloc(n + 1)?;
    ctx.ck(unsafe { kmx_sketch_lookup_reads(ctx.0, &r, ptr::null(), k as u32, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed,
                                            d_est.as_mut_ptr::<u8>()) })?;
    d_est.download::<u8>(n)
}

/// The same for k in 33..=64 (`kmx_sketch_lookup_reads2`).
pub fn sketch_lookup_reads2(ctx: &HipContext, sketch: &Sketch<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8)
                            -> Result<Vec<u8>, KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    let n = n_reads as usize * (read_len as usize + 1).saturating_sub(k as usize);
    let d_est = ctx.alloc(n + 1)?;
    ctx.ck(unsafe { kmx_sketch_lookup_reads2(ctx.0, &r, ptr::null(), k as u32, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed,
                                             d_est.as_mut_ptr::<u8>()) })?;
    d_est.download::<u8>(n)
}

/// `acc` += `other`, cellwise and saturating (`kmx_sketch_merge` with the output on its first input): sketches of disjoint batches
/// with one size and seed merge into the sketch of their union, bit for bit.
pub fn sketch_merge(ctx: &HipContext, acc: &Sketch<'_>, other: &Sketch<'_>) -> Result<(), KmxError> {
    assert!(acc.log2_blocks == other.log2_blocks && acc.seed == other.seed, "sketches of different size or seed do not merge");
    ctx.ck(unsafe { kmx_sketch_merge(ctx.0, acc.cells.as_ptr::<u8>(), other.cells.as_ptr::<u8>(), acc.log2_blocks, acc.cells.as_mut_ptr::<u8>()) })
}

/// How many cells hold each value, 256 bins (`kmx_sketch_stats`); `1 - bins[0] / cells` is the fill a sketch is sized by.
pub fn sketch_stats(ctx: &HipContext, sketch: &Sketch<'_>) -> Result<Vec<u64>, KmxError> {
    let d_hist = ctx.alloc(8 * 256)?;
    ctx.ck(unsafe { kmx_memset(ctx.0, d_hist.as_mut_ptr(), 0, d_hist.len()) })?;
    ctx.ck(unsafe { kmx_sketch_stats(ctx.0, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, d_hist.as_mut_ptr::<u64>()) })?;
    d_hist.download::<u64>(256)
}

/// `count_canonical` of the windows whose estimate in `sketch` is at least `min_est` (`kmx_count_canonical_min`): with a sketch that
/// has seen every batch, the k-mers that can occur `min_est` times in all of them.
pub fn count_canonical_min(ctx: &HipContext, sketch: &Sketch<'_>, min_est: u32, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8,
                           d_kmers: &DeviceBuf<'_>, d_counts: &DeviceBuf<'_>, max_distinct: u64) -> Result<u64, KmxError> {
    assert!(max_distinct as u128 * 8 <= d_kmers.len().min(d_counts.len()) as u128, "outputs shorter than max_distinct");
    let r = sketch_reads(d_reads, n_reads, read_len);
    let mut n_distinct = 0u64;
    ctx.ck(unsafe { kmx_count_canonical_min(ctx.0, &r, k as u32, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed, min_est,
                                            d_kmers.as_mut_ptr::<u64>(), d_counts.as_mut_ptr::<u64>(), max_distinct, &mut n_distinct) })?;
    Ok(n_distinct)
}

/// The same for two-word k-mers, k in 33..=64 (`kmx_count_canonical_min2`; `d_kmers2` holds at least `2 * max_distinct` u64).
pub fn count_canonical_min2(ctx: &HipContext, sketch: &Sketch<'_>, min_est: u32, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8,
                            d_kmers2: &DeviceBuf<'_>, d_counts: &DeviceBuf<'_>, max_distinct: u64) -> Result<u64, KmxError> {
    assert!(max_distinct as u128 * 16 <= d_kmers2.len() as u128 && max_distinct as u128 * 8 <= d_counts.len() as u128,
            "outputs shorter than max_distinct");
    let r = sketch_reads(d_reads, n_reads, read_len);
    let mut n_distinct = 0u64;
    ctx.ck(unsafe { kmx_count_canonical_min2(ctx.0, &r, k as u32, sketch.cells.as_ptr::<u8>(), sketch.log2_blocks, sketch.seed, min_est,
                                             d_kmers2.as_mut_ptr::<u64>(), d_counts.as_mut_ptr::<u64>(), max_distinct, &mut n_distinct) })?;
    Ok(n_distinct)
}

// ------------------------------------------------------------------------------------------------ the distinct-key estimator

/// HyperLogLog registers on the device (`kmx_hll_*`, include/kmx.h "the distinct-key estimator"): `1 << log2_regs` bytes, zero when
/// new and accumulated into; a key raises the register named by the top bits of its hash under `seed` to the rank of the rest.
pub struct Hll<'c> {
    pub regs: DeviceBuf<'c>,
    pub log2_regs: u32,
    pub seed: u64,
}

/// Zeroed registers, `2^log2_regs` of them (`4 <= log2_regs <= 24`): a relative standard error of about `1.04 / sqrt(2^log2_regs)`.
pub fn hll_new(ctx: &HipContext, log2_regs: u32, seed: u64) -> Result<Hll<'_>, KmxError> {
    assert!((4..=24).contains(&log2_regs), "log2_regs outside 4..=24");
    let regs = ctx.alloc(1usize << log2_regs)?;
    ctx.ck(unsafe { kmx_memset(ctx.0, regs.as_mut_ptr(), 0, regs.len()) })?;
    Ok(Hll { regs, log2_regs, seed })
}

/// Every valid window of a uniform batch already on the device (`kmx_hll_add`, k in 1..=31).
pub fn hll_add(ctx: &HipContext, hll: &Hll<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8) -> Result<(), KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    ctx.ck(unsafe { kmx_hll_add(ctx.0, &r, k as u32, hll.regs.as_mut_ptr::<u8>(), hll.log2_regs, hll.seed) })
}

/// The same for two-word k-mers, k in 33..=64 (`kmx_hll_add2`).
pub fn hll_add2(ctx: &HipContext, hll: &Hll<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8) -> Result<(), KmxError> {
    let r = sketch_reads(d_reads, n_reads, read_len);
    ctx.ck(unsafe { kmx_hll_add2(ctx.0, &r, k as u32, hll.regs.as_mut_ptr::<u8>(), hll.log2_regs, hll.seed) })
}

/// `n` one-word keys as they are (`kmx_hll_add_words`): a table's keys, or the canonical words of a windows call.
pub fn hll_add_words(ctx: &HipContext, hll: &Hll<'_>, d_words: &DeviceBuf<'_>, n: u64) -> Result<(), KmxError> {
    assert!(n as u128 * 8 <= d_words.len() as u128, "keys shorter than n");
    ctx.ck(unsafe { kmx_hll_add_words(ctx.0, d_words.as_ptr::<u64>(), n, hll.regs.as_mut_ptr::<u8>(), hll.log2_regs, hll.seed) })
}

/// The same for two-word keys, (low, high) pairs (`kmx_hll_add_words2`).
pub fn hll_add_words2(ctx: &HipContext, hll: &Hll<'_>, d_words2: &DeviceBuf<'_>, n: u64) -> Result<(), KmxError> {
    assert!(n as u128 * 16 <= d_words2.len() as u128, "keys shorter than n");
    ctx.ck(unsafe { kmx_hll_add_words2(ctx.0, d_words2.as_ptr::<u64>(), n, hll.regs.as_mut_ptr::<u8>(), hll.log2_regs, hll.seed) })
}

/// `acc` = max(`acc`, `other`), bytewise (`kmx_hll_merge` with the output on its first input): registers of one size and seed merge
/// into the registers of the union of what they saw, bit for bit.
pub fn hll_merge(ctx: &HipContext, acc: &Hll<'_>, other: &Hll<'_>) -> Result<(), KmxError> {
    assert!(acc.log2_regs == other.log2_regs && acc.seed == other.seed, "registers of different size or seed do not merge");
    ctx.ck(unsafe { kmx_hll_merge(ctx.0, acc.regs.as_ptr::<u8>(), other.regs.as_ptr::<u8>(), acc.log2_regs, acc.regs.as_mut_ptr::<u8>()) })
}

/// How many registers hold each value (`kmx_hll_stats`): 64 bins, or with `other` 192 -- those of `hll`, of `other` and of their
/// bytewise maximum, the registers of the union.
pub fn hll_stats(ctx: &HipContext, hll: &Hll<'_>, other: Option<&Hll<'_>>) -> Result<Vec<u64>, KmxError> {
    assert!(other.map_or(true, |o| o.log2_regs == hll.log2_regs && o.seed == hll.seed), "registers of different size or seed do not compare");
    let n = if other.is_some() { 192 } else { 64 };
    let d_hist = ctx.alloc(8 * n)?;
    ctx.ck(unsafe { kmx_memset(ctx.0, d_hist.as_mut_ptr(), 0, d_hist.len()) })?;
    let b = other.map_or(ptr::null(), |o| o.regs.as_ptr::<u8>());
    ctx.ck(unsafe { kmx_hll_stats(ctx.0, hll.regs.as_ptr::<u8>(), b, hll.log2_regs, d_hist.as_mut_ptr::<u64>()) })?;
    d_hist.download::<u64>(n)
}

fn hll_sigma(mut x: f64) -> f64 {
    if x == 1.0 {
        return f64::INFINITY;
    }
    let (mut y, mut z) = (1.0f64, x);
    loop {
        x *= x;
        let z0 = z;
        z += x * y;
        y += y;
        if z == z0 {
            return z;
        }
    }
}

fn hll_tau(mut x: f64) -> f64 {
    if x == 0.0 || x == 1.0 {
        return 0.0;
    }
    let (mut y, mut z) = (1.0f64, 1.0 - x);
    loop {
        x = x.sqrt();
        let z0 = z;
        y *= 0.5;
        z -= (1.0 - x) * (1.0 - x) * y;
        if z == z0 {
            return z / 3.0;
        }
    }
}

/// The number of distinct keys behind registers, from their 64 bins (`hll_stats`): Ertl's improved estimator exactly as include/kmx.h
/// spells it out, in double precision.  All registers zero gives 0.
pub fn hll_estimate(hist: &[u64], log2_regs: u32) -> f64 {
    assert!((4..=24).contains(&log2_regs), "log2_regs outside 4..=24");
    let q = (64 - log2_regs) as usize;
    assert!(hist.len() >= q + 2, "fewer bins than 66 - log2_regs");
    let m = (1u64 << log2_regs) as f64;
    let mut z = m * hll_tau(1.0 - hist[q + 1] as f64 / m);
    for j in (1..=q).rev() {
        z = 0.5 * (z + hist[j] as f64);
    }
    z += m * hll_sigma(hist[0] as f64 / m);
    m * m / (2.0 * std::f64::consts::LN_2) / z
}

/// The smallest `log2_blocks` in 0..=32 at which a counting sketch that `n_distinct` keys were added to is at most `fill` full
/// (the occupancy of a 16-cell row, `1 - exp(-n / (16 * 2^b))`): what `sketch_new` is sized by from `hll_estimate`.
pub fn hll_sketch_log2_blocks(n_distinct: f64, fill: f64) -> u32 {
    assert!(fill > 0.0 && fill < 1.0, "fill outside (0, 1)");
    (0..32u32).find(|&b| 1.0 - (-n_distinct / (16.0 * (1u64 << b) as f64)).exp() <= fill).unwrap_or(32)
}

/// A count table on the device: `keys` (`words` u64 per entry: 1 for k <= 31, 2 for k in 33..=64; ascending, distinct), one u64
/// count per entry in `counts` (`None`: membership only, where a call allows it), `n` entries.
#[derive(Clone, Copy)]
pub struct CountTable<'a> {
    pub keys: &'a DeviceBuf<'a>,
    pub counts: Option<&'a DeviceBuf<'a>>,
    pub n: u64,
}

impl CountTable<'_> {
    fn check(&self, words: u64) {
        assert!(self.n as u128 * 8 * words as u128 <= self.keys.len() as u128, "table keys shorter than the entry count");
        if let Some(c) = self.counts {
            assert!(self.n as u128 * 8 <= c.len() as u128, "table counts shorter than the entry count");
        }
    }
    fn counts_ptr(&self) -> *const u64 {
        self.counts.map_or(ptr::null(), |c| c.as_ptr::<u64>())
    }
}

/// The count of every query word in a table (`kmx_count_lookup`): `d_out[i]` = the count of `d_query[i]`, 0 if absent or if its
/// flag (`d_flags`, one byte per query, optional) lacks `KMX_WIN_VALID`.  `d_out` may be `d_query` itself.
pub fn count_lookup(ctx: &HipContext, table: CountTable<'_>, k: u8, d_query: &DeviceBuf<'_>, d_flags: Option<&DeviceBuf<'_>>, n_query: u64,
                    d_out: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(1);
    assert!(n_query as u128 * 8 <= d_query.len().min(d_out.len()) as u128, "queries or answers shorter than n_query");
    assert!(d_flags.map_or(true, |f| n_query as u128 <= f.len() as u128), "flags shorter than n_query");
    let flags = d_flags.map_or(ptr::null(), |f| f.as_ptr::<u8>());
    ctx.ck(unsafe { kmx_count_lookup(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, d_query.as_ptr::<u64>(), flags, n_query,
                                     d_out.as_mut_ptr::<u64>()) })
}

/// The same for two-word keys (`kmx_count_lookup2`): 16 bytes per key and per query, 8 per answer.
pub fn count_lookup2(ctx: &HipContext, table: CountTable<'_>, k: u8, d_query2: &DeviceBuf<'_>, d_flags: Option<&DeviceBuf<'_>>, n_query: u64,
                     d_out: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(2);
    assert!(n_query as u128 * 16 <= d_query2.len() as u128 && n_query as u128 * 8 <= d_out.len() as u128, "queries or answers shorter than n_query");
    assert!(d_flags.map_or(true, |f| n_query as u128 <= f.len() as u128), "flags shorter than n_query");
    let flags = d_flags.map_or(ptr::null(), |f| f.as_ptr::<u8>());
    ctx.ck(unsafe { kmx_count_lookup2(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, d_query2.as_ptr::<u64>(), flags, n_query,
                                      d_out.as_mut_ptr::<u64>()) })
}

/// The count, in a table, of the canonical k-mer of every window of a uniform batch on the device (`kmx_count_lookup_reads`):
/// `d_out[r * (read_len - k + 1) + p]`, 0 for a window with an invalid byte.  Returns the number of windows.
pub fn count_lookup_reads(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>,
                          d_out: &DeviceBuf<'_>) -> Result<u64, KmxError> {
    table.check(1);
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    let n_win = n_reads * (read_len as u64 + 1).saturating_sub(k as u64);
    assert!(n_win as u128 * 8 <= d_out.len() as u128, "answers shorter than the batch's windows");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_lookup_reads(ctx.0, &r, ptr::null(), k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n,
                                           d_out.as_mut_ptr::<u64>()) })?;
    Ok(n_win)
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_lookup_reads2`).
pub fn count_lookup_reads2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>,
                           d_out: &DeviceBuf<'_>) -> Result<u64, KmxError> {
    table.check(2);
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    let n_win = n_reads * (read_len as u64 + 1).saturating_sub(k as u64);
    assert!(n_win as u128 * 8 <= d_out.len() as u128, "answers shorter than the batch's windows");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_lookup_reads2(ctx.0, &r, ptr::null(), k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n,
                                            d_out.as_mut_ptr::<u64>()) })?;
    Ok(n_win)
}

/// Per-read abundance statistics of a uniform batch against a table (`kmx_count_read_stats`): `KMX_RS_WORDS` u64 per read in
/// `d_stats` (row `r` at word `8 * r`; the words are `KMX_RS_N_VALID` .. `KMX_RS_SPAN`) -- the valid, present and solid
/// (count >= `solid_min`) windows, min, max, sum and upper median of the counts, and the longest run of solid windows.  Every row is
/// written.
pub fn count_read_stats(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, solid_min: u64,
                        d_stats: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(1);
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(n_reads as u128 * 8 * KMX_RS_WORDS as u128 <= d_stats.len() as u128, "rows shorter than the batch's reads");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_read_stats(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, solid_min,
                                         d_stats.as_mut_ptr::<u64>()) })
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_read_stats2`).
pub fn count_read_stats2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, solid_min: u64,
                         d_stats: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(2);
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(n_reads as u128 * 8 * KMX_RS_WORDS as u128 <= d_stats.len() as u128, "rows shorter than the batch's reads");
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_read_stats2(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, solid_min,
                                          d_stats.as_mut_ptr::<u64>()) })
}

/// Substitution errors of a uniform batch repaired against a table (`kmx_count_correct_reads`): `d_out` receives the reads -- every
/// byte of the batch is written -- with the bases replaced that no window of count >= `solid_min` covers, at least `min_cover`
/// (1 ..= k) valid windows do, and exactly one other base makes all of those windows solid.  `d_fixes`, when given, receives
/// `KMX_CR_WORDS` u64 per read (`KMX_CR_N_WEAK` .. `KMX_CR_N_AMBIGUOUS`).  Decisions are taken against the original bytes: `d_out`
/// must not overlap `d_reads` (`KMX_E_ARG`).
pub fn count_correct_reads(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, solid_min: u64,
                           min_cover: u32, d_out: &DeviceBuf<'_>, d_fixes: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(1);
    let fixes = correct_outputs(d_reads, n_reads, read_len, d_out, d_fixes);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_correct_reads(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, solid_min, min_cover,
                                            d_out.as_mut_ptr::<u8>(), fixes) })
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_correct_reads2`).
pub fn count_correct_reads2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, solid_min: u64,
                            min_cover: u32, d_out: &DeviceBuf<'_>, d_fixes: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(2);
    let fixes = correct_outputs(d_reads, n_reads, read_len, d_out, d_fixes);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_correct_reads2(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, solid_min, min_cover,
                                             d_out.as_mut_ptr::<u8>(), fixes) })
}

// the sizes count_correct_reads(2) ask of their buffers; the rows' pointer, null when they are not wanted
fn correct_outputs(d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_out: &DeviceBuf<'_>, d_fixes: Option<&DeviceBuf<'_>>) -> *mut u64 {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(n_reads as u128 * read_len as u128 <= d_out.len() as u128, "output shorter than the batch's reads");
    match d_fixes {
        Some(f) => {
            assert!(n_reads as u128 * 8 * KMX_CR_WORDS as u128 <= f.len() as u128, "rows shorter than the batch's reads");
            f.as_mut_ptr::<u64>()
        }
        None => ptr::null_mut(),
    }
}

/// The pairwise matrix and the spectrum of a coloured table (`kmx_count_color_matrix`): a table whose u64 per key -- `d_colors`,
/// in the place of the counts -- is a bit mask of the samples (colours `0 .. n_colors`, at most 64) that hold the key.  `d_matrix`
/// receives `n_colors * n_colors` u64, row-major: the entries that hold colours i and j (the diagonal = the samples' sizes);
/// `d_spectrum`, when given, `n_colors + 1` u64: the entries with exactly j colours.  Only the low `n_colors` bits of a mask count.
/// Both outputs are overwritten.
pub fn count_color_matrix(ctx: &HipContext, d_colors: &DeviceBuf<'_>, n: u64, n_colors: u32, d_matrix: &DeviceBuf<'_>,
                          d_spectrum: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    assert!(n as u128 * 8 <= d_colors.len() as u128, "masks shorter than the entry count");
    assert!(n_colors as u128 * n_colors as u128 * 8 <= d_matrix.len() as u128, "matrix shorter than n_colors * n_colors");
    assert!(d_spectrum.map_or(true, |s| (n_colors as u128 + 1) * 8 <= s.len() as u128), "spectrum shorter than n_colors + 1");
    let spectrum = d_spectrum.map_or(ptr::null_mut(), |s| s.as_mut_ptr::<u64>());
    ctx.ck(unsafe { kmx_count_color_matrix(ctx.0, d_colors.as_ptr::<u64>(), n, n_colors, d_matrix.as_mut_ptr::<u64>(), spectrum) })
}

/// Which samples each read of a uniform batch is compatible with (`kmx_count_read_colors`): `table.counts` holds the colour masks
/// of a coloured table (required unless the table is empty).  `d_rows` receives `KMX_RC_WORDS` u64 per read (`KMX_RC_N_VALID` ..
/// `KMX_RC_N_SWITCH`): the valid, hit and single-colour windows, the AND and the OR of the hit windows' masks, the colours that at
/// least `thr_num / thr_den` of the valid windows carry, the best colour with its hit count, and the mask changes between
/// neighbouring hit windows.  `d_hits`, when given, receives `n_colors` u32 per read: the hit windows per colour.  Every row is written.
pub fn count_read_colors(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, n_colors: u32,
                         thr_num: u32, thr_den: u32, d_rows: &DeviceBuf<'_>, d_hits: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(1);
    let hits = read_colors_outputs(d_reads, n_reads, read_len, n_colors, d_rows, d_hits);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_read_colors(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, n_colors, thr_num, thr_den,
                                          d_rows.as_mut_ptr::<u64>(), hits) })
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_read_colors2`).
pub fn count_read_colors2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>, n_colors: u32,
                          thr_num: u32, thr_den: u32, d_rows: &DeviceBuf<'_>, d_hits: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(2);
    let hits = read_colors_outputs(d_reads, n_reads, read_len, n_colors, d_rows, d_hits);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    ctx.ck(unsafe { kmx_count_read_colors2(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, n_colors, thr_num, thr_den,
                                           d_rows.as_mut_ptr::<u64>(), hits) })
}

// the sizes count_read_colors(2) ask of their buffers; the hit counts' pointer, null when they are not wanted
fn read_colors_outputs(d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, n_colors: u32, d_rows: &DeviceBuf<'_>,
                       d_hits: Option<&DeviceBuf<'_>>) -> *mut u32 {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(n_reads as u128 * 8 * KMX_RC_WORDS as u128 <= d_rows.len() as u128, "rows shorter than the batch's reads");
    match d_hits {
        Some(h) => {
            assert!(n_reads as u128 * 4 * n_colors as u128 <= h.len() as u128, "hit counts shorter than the batch's reads");
            h.as_mut_ptr::<u32>()
        }
        None => ptr::null_mut(),
    }
}

/// The abundance spectrum of a table's counts (`kmx_count_spectrum`): `n_bins` bins, bin c = how many entries have count c, the last
/// bin everything at or above it.
pub fn count_spectrum(ctx: &HipContext, d_counts: &DeviceBuf<'_>, n: u64, n_bins: usize) -> Result<Vec<u64>, KmxError> {
    assert!(n as u128 * 8 <= d_counts.len() as u128, "counts shorter than the entry count");
    let d_bins = ctx.upload(&vec![0u8; 8 * n_bins.max(1)])?;
    ctx.ck(unsafe { kmx_count_spectrum(ctx.0, d_counts.as_ptr::<u64>(), n, n_bins as u64, d_bins.as_mut_ptr::<u64>()) })?;
    d_bins.download::<u64>(n_bins)
}

/// The table as the node set of a de Bruijn graph (`kmx_count_adjacency`, k in 2..=31): `d_edges[i]` = one bit per neighbour of
/// entry i that is a present entry (bit c: the successor ending in base c, bit 4 + c: the predecessor starting with it); optional
/// `d_flips` (the same bits: the neighbour is stored as the reverse complement) and `d_nbr` (8 u64 per entry: the neighbour's
/// table index, `KMX_NO_ENTRY` where there is no edge).  An entry is present if its count is at least `min_count`.
pub fn count_adjacency(ctx: &HipContext, table: CountTable<'_>, k: u8, min_count: u64, d_edges: &DeviceBuf<'_>, d_flips: Option<&DeviceBuf<'_>>,
                       d_nbr: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(1);
    let (flips, nbr) = adjacency_outputs(table.n, d_edges, d_flips, d_nbr);
    ctx.ck(unsafe { kmx_count_adjacency(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, min_count,
                                        d_edges.as_mut_ptr::<u8>(), flips, nbr) })
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_adjacency2`).
pub fn count_adjacency2(ctx: &HipContext, table: CountTable<'_>, k: u8, min_count: u64, d_edges: &DeviceBuf<'_>, d_flips: Option<&DeviceBuf<'_>>,
                        d_nbr: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    table.check(2);
    let (flips, nbr) = adjacency_outputs(table.n, d_edges, d_flips, d_nbr);
    ctx.ck(unsafe { kmx_count_adjacency2(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, min_count,
                                         d_edges.as_mut_ptr::<u8>(), flips, nbr) })
}

fn adjacency_outputs(n: u64, d_edges: &DeviceBuf<'_>, d_flips: Option<&DeviceBuf<'_>>, d_nbr: Option<&DeviceBuf<'_>>) -> (*mut u8, *mut u64) {
    assert!(n as u128 <= d_edges.len() as u128, "edge bytes shorter than the entry count");
    assert!(d_flips.map_or(true, |f| n as u128 <= f.len() as u128), "flip bytes shorter than the entry count");
    assert!(d_nbr.map_or(true, |b| n as u128 * 64 <= b.len() as u128), "neighbour indices shorter than 8 per entry");
    (d_flips.map_or(ptr::null_mut(), |f| f.as_mut_ptr::<u8>()), d_nbr.map_or(ptr::null_mut(), |b| b.as_mut_ptr::<u64>()))
}

/// How many entries have each edge byte (`kmx_count_edge_histogram`): 256 bins, from which every degree statistic follows.
pub fn count_edge_histogram(ctx: &HipContext, d_edges: &DeviceBuf<'_>, n: u64) -> Result<Vec<u64>, KmxError> {
    assert!(n as u128 <= d_edges.len() as u128, "edge bytes shorter than the entry count");
    let d_bins = ctx.upload(&vec![0u8; 8 * 256])?;
    ctx.ck(unsafe { kmx_count_edge_histogram(ctx.0, d_edges.as_ptr::<u8>(), n, d_bins.as_mut_ptr::<u64>()) })?;
    d_bins.download::<u64>(256)
}

/// Where the non-branching paths end (`kmx_count_unitig_ends`), from the three outputs of `count_adjacency(2)`: bit 0 of
/// `d_ends[i]` = the successor side of entry i is an end, bit 1 = its predecessor side is.
pub fn count_unitig_ends(ctx: &HipContext, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>, d_nbr: &DeviceBuf<'_>, n: u64,
                         d_ends: &DeviceBuf<'_>) -> Result<(), KmxError> {
    assert!(n as u128 <= d_edges.len().min(d_flips.len()).min(d_ends.len()) as u128, "a byte array shorter than the entry count");
    assert!(n as u128 * 64 <= d_nbr.len() as u128, "neighbour indices shorter than 8 per entry");
    ctx.ck(unsafe { kmx_count_unitig_ends(ctx.0, d_edges.as_ptr::<u8>(), d_flips.as_ptr::<u8>(), d_nbr.as_ptr::<u64>(), n,
                                          d_ends.as_mut_ptr::<u8>()) })
}

/// The device arrays `count_unitigs(2)` fills: `d_nodes` (n u64), `d_offsets` (n + 1 u64), optional `d_circular` (n bytes) and
/// `d_count_sums` (n u64).
pub struct UnitigOutputs<'a> {
    pub d_nodes: &'a DeviceBuf<'a>,
    pub d_offsets: &'a DeviceBuf<'a>,
    pub d_circular: Option<&'a DeviceBuf<'a>>,
    pub d_count_sums: Option<&'a DeviceBuf<'a>>,
}

impl UnitigOutputs<'_> {
    fn check(&self, n: u64) -> (*mut u8, *mut u64) {
        assert!(n as u128 * 8 <= self.d_nodes.len() as u128, "unitig nodes shorter than the entry count");
        assert!((n as u128 + 1) * 8 <= self.d_offsets.len() as u128, "unitig offsets shorter than the entry count + 1");
        assert!(self.d_circular.map_or(true, |c| n as u128 <= c.len() as u128), "circular flags shorter than the entry count");
        assert!(self.d_count_sums.map_or(true, |c| n as u128 * 8 <= c.len() as u128), "count sums shorter than the entry count");
        (self.d_circular.map_or(ptr::null_mut(), |c| c.as_mut_ptr::<u8>()), self.d_count_sums.map_or(ptr::null_mut(), |c| c.as_mut_ptr::<u64>()))
    }
}

fn unitig_inputs(n: u64, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>, d_nbr: &DeviceBuf<'_>) {
    assert!(n as u128 <= d_edges.len().min(d_flips.len()) as u128, "a byte array shorter than the entry count");
    assert!(n as u128 * 64 <= d_nbr.len() as u128, "neighbour indices shorter than 8 per entry");
}

/// The unitigs of the table's de Bruijn graph (`kmx_count_unitigs`, k in 2..=31) from the three outputs of `count_adjacency` made
/// with the same `min_count`: the oriented nodes `2 * entry + o` of the canonical unitigs one after another, their offsets, circular
/// flags and count sums (include/kmx.h has the definitions).  Returns (unitigs, nodes).  Synchronous.
pub fn count_unitigs(ctx: &HipContext, table: CountTable<'_>, k: u8, min_count: u64, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>,
                     d_nbr: &DeviceBuf<'_>, out: &UnitigOutputs<'_>) -> Result<(u64, u64), KmxError> {
    table.check(1);
    unitig_inputs(table.n, d_edges, d_flips, d_nbr);
    let (circular, sums) = out.check(table.n);
    let (mut n_unitigs, mut n_nodes) = (0u64, 0u64);
    ctx.ck(unsafe { kmx_count_unitigs(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, min_count, d_edges.as_ptr::<u8>(),
                                      d_flips.as_ptr::<u8>(), d_nbr.as_ptr::<u64>(), out.d_nodes.as_mut_ptr::<u64>(),
                                      out.d_offsets.as_mut_ptr::<u64>(), circular, sums, &mut n_unitigs, &mut n_nodes) })?;
    Ok((n_unitigs, n_nodes))
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_unitigs2`).
pub fn count_unitigs2(ctx: &HipContext, table: CountTable<'_>, k: u8, min_count: u64, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>,
                      d_nbr: &DeviceBuf<'_>, out: &UnitigOutputs<'_>) -> Result<(u64, u64), KmxError> {
    table.check(2);
    unitig_inputs(table.n, d_edges, d_flips, d_nbr);
    let (circular, sums) = out.check(table.n);
    let (mut n_unitigs, mut n_nodes) = (0u64, 0u64);
    ctx.ck(unsafe { kmx_count_unitigs2(ctx.0, table.keys.as_ptr::<u64>(), table.counts_ptr(), table.n, k as u32, min_count, d_edges.as_ptr::<u8>(),
                                       d_flips.as_ptr::<u8>(), d_nbr.as_ptr::<u64>(), out.d_nodes.as_mut_ptr::<u64>(),
                                       out.d_offsets.as_mut_ptr::<u64>(), circular, sums, &mut n_unitigs, &mut n_nodes) })?;
    Ok((n_unitigs, n_nodes))
}

/// The bases of the unitigs, ASCII (`kmx_count_unitig_sequences`): unitig u starts at byte `offsets[u] + u * (k - 1)` of `d_seq`,
/// which holds `n_nodes + n_unitigs * (k - 1)` bytes.  Asynchronous.
pub fn count_unitig_sequences(ctx: &HipContext, table: CountTable<'_>, k: u8, d_nodes: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64,
                              n_nodes: u64, d_seq: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(1);
    unitig_sequence_arrays(k, d_nodes, d_offsets, n_unitigs, n_nodes, d_seq);
    ctx.ck(unsafe { kmx_count_unitig_sequences(ctx.0, table.keys.as_ptr::<u64>(), table.n, k as u32, d_nodes.as_ptr::<u64>(),
                                               d_offsets.as_ptr::<u64>(), n_unitigs, d_seq.as_mut_ptr::<u8>()) })
}

/// The same for two-word keys (`kmx_count_unitig_sequences2`).
pub fn count_unitig_sequences2(ctx: &HipContext, table: CountTable<'_>, k: u8, d_nodes: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64,
                               n_nodes: u64, d_seq: &DeviceBuf<'_>) -> Result<(), KmxError> {
    table.check(2);
    unitig_sequence_arrays(k, d_nodes, d_offsets, n_unitigs, n_nodes, d_seq);
    ctx.ck(unsafe { kmx_count_unitig_sequences2(ctx.0, table.keys.as_ptr::<u64>(), table.n, k as u32, d_nodes.as_ptr::<u64>(),
                                                d_offsets.as_ptr::<u64>(), n_unitigs, d_seq.as_mut_ptr::<u8>()) })
}

fn unitig_sequence_arrays(k: u8, d_nodes: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64, n_nodes: u64, d_seq: &DeviceBuf<'_>) {
    assert!(n_nodes as u128 * 8 <= d_nodes.len() as u128, "unitig nodes shorter than the node count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!(n_nodes as u128 + n_unitigs as u128 * (k as u128 - 1) <= d_seq.len() as u128, "sequence bytes shorter than nodes + unitigs * (k - 1)");
}

/// Where each of the table's `n` entries sits in the unitigs (`kmx_count_unitig_index`): `d_place[i]` =
/// `((p + 1) << 3) | (last << 2) | (first << 1) | o` for the entry `d_nodes[p]` names, `KMX_PLACE_NONE` for an entry in no unitig.
/// It serves the lookups as their counts array.  One call for both key widths.  Asynchronous.
pub fn count_unitig_index(ctx: &HipContext, d_nodes: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64, n_nodes: u64, n: u64,
                          d_place: &DeviceBuf<'_>) -> Result<(), KmxError> {
    assert!(n_nodes as u128 * 8 <= d_nodes.len() as u128, "unitig nodes shorter than the node count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!(n as u128 * 8 <= d_place.len() as u128, "places shorter than the entry count");
    ctx.ck(unsafe { kmx_count_unitig_index(ctx.0, d_nodes.as_ptr::<u64>(), d_offsets.as_ptr::<u64>(), n_unitigs, n, d_place.as_mut_ptr::<u64>()) })
}

/// The device arrays `count_read_paths(2)` fills: `d_path_offsets` (n_reads + 1 u64) and `d_segments` (`KMX_PATH_WORDS` u64 per
/// segment, room for `max_segments`).
pub struct PathOutputs<'a> {
    pub d_path_offsets: &'a DeviceBuf<'a>,
    pub d_segments: &'a DeviceBuf<'a>,
    pub max_segments: u64,
}

fn path_arrays(table: &CountTable<'_>, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>,
               n_unitigs: u64, out: Option<&PathOutputs<'_>>) -> (*mut u64, *mut u64, u64) {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(table.n as u128 * 8 <= d_place.len() as u128, "places shorter than the entry count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    out.map_or((ptr::null_mut(), ptr::null_mut(), 0), |o| {
        assert!((n_reads as u128 + 1) * 8 <= o.d_path_offsets.len() as u128, "path offsets shorter than the batch's reads + 1");
        assert!(o.max_segments as u128 * 8 * KMX_PATH_WORDS as u128 <= o.d_segments.len() as u128, "segments shorter than max_segments");
        (o.d_path_offsets.as_mut_ptr::<u64>(), o.d_segments.as_mut_ptr::<u64>(), o.max_segments)
    })
}

/// The segments of every read of a uniform batch over the unitigs of a table (`kmx_count_read_paths`, k in 2..=31): one record of
/// `KMX_PATH_WORDS` u64 (`KMX_PATH_READ` .. `KMX_PATH_POS`) per maximal run of consecutive windows that walk one unitig in one
/// direction, ordered by read, then by start; read r owns the segments `path_offsets[r] .. path_offsets[r + 1]`.  `table.counts` is
/// not read; `d_place` is what `count_unitig_index` wrote for `d_offsets` / `n_unitigs`.  `out = None` counts only.  Returns the
/// number of segments; Err(KMX_E_NOMEM) if there are more than `max_segments` (the path offsets are written all the same).
/// Synchronous.
pub fn count_read_paths(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>,
                        d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64, out: Option<&PathOutputs<'_>>) -> Result<u64, KmxError> {
    table.check(1);
    let (path_offsets, segments, max_segments) = path_arrays(&table, d_reads, n_reads, read_len, d_place, d_offsets, n_unitigs, out);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut n_segments = 0u64;
    ctx.ck(unsafe { kmx_count_read_paths(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.n, d_place.as_ptr::<u64>(), d_offsets.as_ptr::<u64>(),
                                         n_unitigs, path_offsets, segments, max_segments, &mut n_segments) })?;
    Ok(n_segments)
}

/// The same for two-word keys, k in 33..=64 (`kmx_count_read_paths2`).
pub fn count_read_paths2(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, table: CountTable<'_>,
                         d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64, out: Option<&PathOutputs<'_>>) -> Result<u64, KmxError> {
    table.check(2);
    let (path_offsets, segments, max_segments) = path_arrays(&table, d_reads, n_reads, read_len, d_place, d_offsets, n_unitigs, out);
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut n_segments = 0u64;
    ctx.ck(unsafe { kmx_count_read_paths2(ctx.0, &r, k as u32, table.keys.as_ptr::<u64>(), table.n, d_place.as_ptr::<u64>(), d_offsets.as_ptr::<u64>(),
                                          n_unitigs, path_offsets, segments, max_segments, &mut n_segments) })?;
    Ok(n_segments)
}

/// The device arrays `count_unitig_links` fills: `d_link_offsets` (2 * n_unitigs + 1 u64) and `d_links` (room for `max_links` u64).
pub struct LinkOutputs<'a> {
    pub d_link_offsets: &'a DeviceBuf<'a>,
    pub d_links: &'a DeviceBuf<'a>,
    pub max_links: u64,
}

/// The links between the oriented unitigs `t = 2 * u + s` of a table's de Bruijn graph (`kmx_count_unitig_links`): t owns
/// `d_links[d_link_offsets[t] .. d_link_offsets[t + 1]]`, at most four targets `t'`, each an overlap of k - 1 bases (include/kmx.h
/// has the rule).  `d_edges` / `d_flips` / `d_nbr` are `count_adjacency`'s outputs for the table's `n` entries, `d_nodes` /
/// `d_offsets` `count_unitigs`' and `d_place` `count_unitig_index`'s.  One call for both key widths.  `out = None` counts only.
/// Returns the number of links; Err(KMX_E_NOMEM) if there are more than `max_links` (the offsets are written all the same).
/// Synchronous.
pub fn count_unitig_links(ctx: &HipContext, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>, d_nbr: &DeviceBuf<'_>, n: u64, d_nodes: &DeviceBuf<'_>,
                          d_offsets: &DeviceBuf<'_>, n_unitigs: u64, n_nodes: u64, d_place: &DeviceBuf<'_>, out: Option<&LinkOutputs<'_>>)
                          -> Result<u64, KmxError> {
    unitig_inputs(n, d_edges, d_flips, d_nbr);
    assert!(n_nodes as u128 * 8 <= d_nodes.len() as u128, "unitig nodes shorter than the node count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!(n as u128 * 8 <= d_place.len() as u128, "places shorter than the entry count");
    let (link_offsets, links, max_links) = out.map_or((ptr::null_mut(), ptr::null_mut(), 0), |o| {
        assert!((2 * n_unitigs as u128 + 1) * 8 <= o.d_link_offsets.len() as u128, "link offsets shorter than twice the unitig count + 1");
        assert!(o.max_links as u128 * 8 <= o.d_links.len() as u128, "links shorter than max_links");
        (o.d_link_offsets.as_mut_ptr::<u64>(), o.d_links.as_mut_ptr::<u64>(), o.max_links)
    });
    let mut n_links = 0u64;
    ctx.ck(unsafe { kmx_count_unitig_links(ctx.0, d_edges.as_ptr::<u8>(), d_flips.as_ptr::<u8>(), d_nbr.as_ptr::<u64>(), n, d_nodes.as_ptr::<u64>(),
                                           d_offsets.as_ptr::<u64>(), n_unitigs, d_place.as_ptr::<u64>(), link_offsets, links, max_links,
                                           &mut n_links) })?;
    Ok(n_links)
}

fn select_arrays(table: &CountTable<'_>, d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64, d_keep: &DeviceBuf<'_>) {
    assert!(table.n as u128 * 8 <= d_place.len() as u128, "places shorter than the entry count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!(n_unitigs as u128 <= d_keep.len() as u128, "keep bytes shorter than the unitig count");
}

/// The entries of a table that lie in a unitig `u` with `d_keep[u] != 0` (one byte per unitig), order kept
/// (`kmx_count_unitig_select`): a table again.  `d_place` is what `count_unitig_index` wrote for `d_offsets` / `n_unitigs`; an
/// entry in no unitig is dropped.  The outputs hold at least `max_out` entries; returns how many were kept, Err(KMX_E_NOMEM) if there
/// are more than `max_out`.
pub fn count_unitig_select(ctx: &HipContext, table: CountTable<'_>, d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64,
                           d_keep: &DeviceBuf<'_>, d_kmers_out: &DeviceBuf<'_>, d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    table.check(1);
    let counts = table.counts.expect("count_unitig_select needs the table's counts");
    select_arrays(&table, d_place, d_offsets, n_unitigs, d_keep);
    assert!(max_out as u128 * 8 <= d_kmers_out.len().min(d_counts_out.len()) as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_unitig_select(ctx.0, table.keys.as_ptr::<u64>(), counts.as_ptr::<u64>(), table.n, d_place.as_ptr::<u64>(),
                                            d_offsets.as_ptr::<u64>(), n_unitigs, d_keep.as_ptr::<u8>(), d_kmers_out.as_mut_ptr::<u64>(),
                                            d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// The same for two-word keys (`kmx_count_unitig_select2`): `d_kmers2_out` holds at least `2 * max_out` u64.
pub fn count_unitig_select2(ctx: &HipContext, table: CountTable<'_>, d_place: &DeviceBuf<'_>, d_offsets: &DeviceBuf<'_>, n_unitigs: u64,
                            d_keep: &DeviceBuf<'_>, d_kmers2_out: &DeviceBuf<'_>, d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    table.check(2);
    let counts = table.counts.expect("count_unitig_select2 needs the table's counts");
    select_arrays(&table, d_place, d_offsets, n_unitigs, d_keep);
    assert!(max_out as u128 * 16 <= d_kmers2_out.len() as u128 && max_out as u128 * 8 <= d_counts_out.len() as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_unitig_select2(ctx.0, table.keys.as_ptr::<u64>(), counts.as_ptr::<u64>(), table.n, d_place.as_ptr::<u64>(),
                                             d_offsets.as_ptr::<u64>(), n_unitigs, d_keep.as_ptr::<u8>(), d_kmers2_out.as_mut_ptr::<u64>(),
                                             d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// The parameters of `count_unitig_clean` (include/kmx.h has the rule): a limit of 0 turns its rule off; `tip_num == 0` makes the tip
/// rule topological, otherwise a dead end goes if its mean count per node is below `tip_num / tip_den` of a sibling's.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct CleanRule {
    pub tip_max_nodes: u64,
    pub tip_num: u32,
    pub tip_den: u32,
    pub bubble_max_nodes: u64,
    pub bubble_max_diff: u64,
    pub island_max_nodes: u64,
}

impl CleanRule {
    /// The choices of the Python layer for k-mers of k bases: tips of at most k nodes at ratio 1/1, bubbles whose branches have at most
    /// 2 k nodes and differ by at most 4, islands kept.  Choices, not measurements.
    pub fn for_k(k: u8) -> CleanRule {
        CleanRule { tip_max_nodes: k as u64, tip_num: 1, tip_den: 1, bubble_max_nodes: 2 * k as u64, bubble_max_diff: 4, island_max_nodes: 0 }
    }
}

/// Which unitigs to drop to clean the compacted graph (`kmx_count_unitig_clean`): one keep byte per unitig into `d_keep`, what
/// `count_unitig_select(2)` takes, and the reason (`KMX_CLEAN_KEEP`, `KMX_CLEAN_TIP`, `KMX_CLEAN_BUBBLE`, `KMX_CLEAN_ISLAND`) into
/// `d_reason` if given.  `d_offsets` / `d_circular` / `d_count_sums` are `count_unitigs`' outputs (the latter two may be None: no
/// unitig circular, every mean count 1), `d_link_offsets` / `d_links` / `n_links` `count_unitig_links`'.  One call for both key widths.
/// Asynchronous.
pub fn count_unitig_clean(ctx: &HipContext, d_offsets: &DeviceBuf<'_>, d_circular: Option<&DeviceBuf<'_>>, d_count_sums: Option<&DeviceBuf<'_>>,
                          n_unitigs: u64, d_link_offsets: &DeviceBuf<'_>, d_links: &DeviceBuf<'_>, n_links: u64, rule: CleanRule,
                          d_keep: &DeviceBuf<'_>, d_reason: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!(d_circular.map_or(true, |b| n_unitigs as u128 <= b.len() as u128), "circular flags shorter than the unitig count");
    assert!(d_count_sums.map_or(true, |b| n_unitigs as u128 * 8 <= b.len() as u128), "count sums shorter than the unitig count");
    assert!((2 * n_unitigs as u128 + 1) * 8 <= d_link_offsets.len() as u128, "link offsets shorter than twice the unitig count + 1");
    assert!(n_links as u128 * 8 <= d_links.len() as u128, "links shorter than the link count");
    assert!(n_unitigs as u128 <= d_keep.len() as u128, "keep bytes shorter than the unitig count");
    assert!(d_reason.map_or(true, |b| n_unitigs as u128 <= b.len() as u128), "reason bytes shorter than the unitig count");
    ctx.ck(unsafe { kmx_count_unitig_clean(ctx.0, d_offsets.as_ptr::<u64>(), d_circular.map_or(ptr::null(), |b| b.as_ptr::<u8>()),
                                           d_count_sums.map_or(ptr::null(), |b| b.as_ptr::<u64>()), n_unitigs, d_link_offsets.as_ptr::<u64>(),
                                           d_links.as_ptr::<u64>(), n_links, rule.tip_max_nodes, rule.tip_num, rule.tip_den, rule.bubble_max_nodes,
                                           rule.bubble_max_diff, rule.island_max_nodes, d_keep.as_mut_ptr::<u8>(),
                                           d_reason.map_or(ptr::null_mut(), |b| b.as_mut_ptr::<u8>())) })
}

/// The label and id of a unitig that the mask of `count_unitig_components` leaves out (`KMX_COMPONENT_NONE`).
pub const COMPONENT_NONE: u64 = !0u64;

/// What `count_unitig_components` brings back to the host: the number of components, and the hook / jump rounds the call ran.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ComponentCount {
    pub n_components: u64,
    pub rounds: u32,
}

/// The connected components of the compacted graph (`kmx_count_unitig_components`; include/kmx.h has the rule): into `d_labels`
/// the smallest unitig index of every unitig's component, into `d_ids` (if given) the component's number in ascending order of the
/// labels, into `d_components` (if given, room for `max_components` records of 4 u64) root, unitigs, nodes and count sum of every
/// component.  `d_mask` (if given, a byte per unitig) leaves unitigs out: their label and id are `COMPONENT_NONE`.  `d_offsets` /
/// `d_count_sums` are `count_unitigs`' outputs (either may be None: every unitig one node, every mean count 1), `d_link_offsets` /
/// `d_links` / `n_links` `count_unitig_links`'.  More components than `max_components`: Err(KMX_E_NOMEM) with `d_components`
/// untouched and labels and ids written all the same.  One call for both key widths.  Synchronous.
pub fn count_unitig_components(ctx: &HipContext, d_offsets: Option<&DeviceBuf<'_>>, d_count_sums: Option<&DeviceBuf<'_>>, n_unitigs: u64,
                               d_link_offsets: &DeviceBuf<'_>, d_links: &DeviceBuf<'_>, n_links: u64, d_mask: Option<&DeviceBuf<'_>>,
                               d_labels: &DeviceBuf<'_>, d_ids: Option<&DeviceBuf<'_>>, d_components: Option<&DeviceBuf<'_>>,
                               max_components: u64) -> Result<ComponentCount, KmxError> {
    assert!(d_offsets.map_or(true, |b| (n_unitigs as u128 + 1) * 8 <= b.len() as u128), "unitig offsets shorter than the unitig count + 1");
    assert!(d_count_sums.map_or(true, |b| n_unitigs as u128 * 8 <= b.len() as u128), "count sums shorter than the unitig count");
    assert!((2 * n_unitigs as u128 + 1) * 8 <= d_link_offsets.len() as u128, "link offsets shorter than twice the unitig count + 1");
    assert!(n_links as u128 * 8 <= d_links.len() as u128, "links shorter than the link count");
    assert!(d_mask.map_or(true, |b| n_unitigs as u128 <= b.len() as u128), "mask shorter than the unitig count");
    assert!(n_unitigs as u128 * 8 <= d_labels.len() as u128, "labels shorter than the unitig count");
    assert!(d_ids.map_or(true, |b| n_unitigs as u128 * 8 <= b.len() as u128), "ids shorter than the unitig count");
    assert!(d_components.map_or(true, |b| max_components as u128 * 32 <= b.len() as u128), "records shorter than max_components");
    let mut out = ComponentCount { n_components: 0, rounds: 0 };
    ctx.ck(unsafe { kmx_count_unitig_components(ctx.0, d_offsets.map_or(ptr::null(), |b| b.as_ptr::<u64>()),
                                                d_count_sums.map_or(ptr::null(), |b| b.as_ptr::<u64>()), n_unitigs, d_link_offsets.as_ptr::<u64>(),
                                                d_links.as_ptr::<u64>(), n_links, d_mask.map_or(ptr::null(), |b| b.as_ptr::<u8>()),
                                                d_labels.as_mut_ptr::<u64>(), d_ids.map_or(ptr::null_mut(), |b| b.as_mut_ptr::<u64>()),
                                                d_components.map_or(ptr::null_mut(), |b| b.as_mut_ptr::<u64>()), max_components,
                                                &mut out.n_components, &mut out.rounds) })?;
    Ok(out)
}

/// How many reads walk each link (`kmx_count_link_support`; include/kmx.h has the rule): for every pair of consecutive segments of one
/// read, the second beginning one base after the first ends, that leaves the exit node of one oriented unitig and enters the entry
/// node of the next, `d_support` (one u64 per link slot) gains 1 at the link's slot and at its mirror's; `d_summary` (`KMX_LS_WORDS`
/// u64) gains the junctions, those that crossed a link and those that did not (0 for paths over the links' own graph).  Both are
/// accumulated into: the caller zeroes them.  `d_segments` / `n_segments` are `count_read_paths(2)`' output, `d_offsets` is
/// `count_unitigs`', `d_link_offsets` / `d_links` / `n_links` `count_unitig_links`'.  One call for both key widths.  Asynchronous.
pub fn count_link_support(ctx: &HipContext, d_segments: &DeviceBuf<'_>, n_segments: u64, d_offsets: &DeviceBuf<'_>, n_unitigs: u64,
                          d_link_offsets: &DeviceBuf<'_>, d_links: &DeviceBuf<'_>, n_links: u64, d_support: &DeviceBuf<'_>,
                          d_summary: &DeviceBuf<'_>) -> Result<(), KmxError> {
    assert!(n_segments as u128 * 32 <= d_segments.len() as u128, "segments shorter than the segment count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!((2 * n_unitigs as u128 + 1) * 8 <= d_link_offsets.len() as u128, "link offsets shorter than twice the unitig count + 1");
    assert!(n_links as u128 * 8 <= d_links.len() as u128, "links shorter than the link count");
    assert!(n_links as u128 * 8 <= d_support.len() as u128, "support shorter than the link count");
    assert!(KMX_LS_WORDS as usize * 8 <= d_summary.len(), "summary shorter than KMX_LS_WORDS words");
    ctx.ck(unsafe { kmx_count_link_support(ctx.0, d_segments.as_ptr::<u64>(), n_segments, d_offsets.as_ptr::<u64>(), n_unitigs,
                                           d_link_offsets.as_ptr::<u64>(), d_links.as_ptr::<u64>(), n_links, d_support.as_mut_ptr::<u64>(),
                                           d_summary.as_mut_ptr::<u64>()) })
}

/// The adjacency without chosen links (`kmx_count_adjacency_cut`): `d_edges_out` (n bytes, not overlapping `d_edges`) = `d_edges` with
/// the edge bit cleared from which link slot l was derived, for every l with `d_cut[l] != 0` (one byte per link slot).  The arrays
/// are those `count_unitig_links` made `d_link_offsets` from; `d_flips` and `d_nbr` go on unchanged with the new edges into
/// `count_unitigs(2)` and `count_unitig_links`.  One call for both key widths.  Asynchronous.
pub fn count_cut_links(ctx: &HipContext, d_edges: &DeviceBuf<'_>, d_flips: &DeviceBuf<'_>, d_nbr: &DeviceBuf<'_>, n: u64, d_nodes: &DeviceBuf<'_>,
                       d_offsets: &DeviceBuf<'_>, n_unitigs: u64, d_place: &DeviceBuf<'_>, d_link_offsets: &DeviceBuf<'_>, n_links: u64,
                       d_cut: &DeviceBuf<'_>, d_edges_out: &DeviceBuf<'_>) -> Result<(), KmxError> {
    assert!(n as u128 <= d_edges.len() as u128 && n as u128 <= d_flips.len() as u128 && n as u128 * 64 <= d_nbr.len() as u128,
            "adjacency shorter than the entry count");
    assert!(n as u128 * 8 <= d_place.len() as u128, "places shorter than the entry count");
    assert!((n_unitigs as u128 + 1) * 8 <= d_offsets.len() as u128, "unitig offsets shorter than the unitig count + 1");
    assert!((2 * n_unitigs as u128 + 1) * 8 <= d_link_offsets.len() as u128, "link offsets shorter than twice the unitig count + 1");
    assert!(n_links as u128 <= d_cut.len() as u128, "cut bytes shorter than the link count");
    assert!(n as u128 <= d_edges_out.len() as u128, "output edges shorter than the entry count");
    ctx.ck(unsafe { kmx_count_adjacency_cut(ctx.0, d_edges.as_ptr::<u8>(), d_flips.as_ptr::<u8>(), d_nbr.as_ptr::<u64>(), n, d_nodes.as_ptr::<u64>(),
                                            d_offsets.as_ptr::<u64>(), n_unitigs, d_place.as_ptr::<u64>(), d_link_offsets.as_ptr::<u64>(), n_links,
                                            d_cut.as_ptr::<u8>(), d_edges_out.as_mut_ptr::<u8>()) })
}

/// The span of every source read for `reads_select` / `reads_gather` (include/kmx.h, "THE SPAN OF A READ"): the span word of read r is
/// word `first_word + r * stride` of `words`, start in its low 32 bits and length in its high 32; `k == 0`: the length counts bases,
/// `k > 0`: windows of k bases.  `ReadSpans { words: &d_stats, first_word: KMX_RS_SPAN as u64, stride: KMX_RS_WORDS as u64, k }` trims
/// every read to its longest run of solid windows straight from the rows of `count_read_stats`.
#[derive(Clone, Copy)]
pub struct ReadSpans<'a> {
    pub words: &'a DeviceBuf<'a>,
    pub first_word: u64,
    pub stride: u64,
    pub k: u32,
}

fn span_args(spans: Option<ReadSpans<'_>>, n_reads: u64) -> (*const u64, u64, u32) {
    match spans {
        None => (ptr::null(), 0, 0),
        Some(s) => {
            assert!(s.stride >= 1, "span stride of 0");
            assert!(n_reads == 0 || (s.first_word as u128 + (n_reads as u128 - 1) * s.stride as u128 + 1) * 8 <= s.words.len() as u128,
                    "span words shorter than the batch's reads");
            (unsafe { s.words.as_ptr::<u64>().add(s.first_word as usize) }, s.stride, s.k)
        }
    }
}

/// The outputs of `reads_select` / `reads_gather`: `bases` (at least `max_bases` bytes), `offsets` (at least `max_reads + 1` u64) and,
/// for `reads_select`, optionally `index` (at least `max_reads` u64: the source read of every output read).
pub struct ReadOutputs<'a> {
    pub bases: &'a DeviceBuf<'a>,
    pub offsets: &'a DeviceBuf<'a>,
    pub index: Option<&'a DeviceBuf<'a>>,
    pub max_reads: u64,
    pub max_bases: u64,
}

fn reads_of(d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>) -> kmx_reads {
    match d_read_offsets {
        Some(o) => {
            assert!((n_reads as u128 + 1) * 8 <= o.len() as u128, "read offsets shorter than the read count + 1");
            kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: o.as_ptr::<u64>() }
        }
        None => {
            assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
            kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() }
        }
    }
}

/// Keep, drop and clip the reads of a batch (`kmx_reads_select`; include/kmx.h has the rule): read r is kept iff `d_keep` is None or
/// its byte r is not 0, and its clip -- the whole read, or its span -- has at least `min_len` bases; the clips are written back to back
/// in source order, a ragged batch again.  Uniform reads (`d_read_offsets` None) or ragged ones.  `out = None` counts only.  Returns
/// (reads kept, bases kept); Err(KMX_E_NOMEM) if they exceed `max_reads` / `max_bases`, with nothing written.  Synchronous.
pub fn reads_select(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                    d_keep: Option<&DeviceBuf<'_>>, spans: Option<ReadSpans<'_>>, min_len: u64, out: Option<&ReadOutputs<'_>>)
                    -> Result<(u64, u64), KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    if let Some(kp) = d_keep {
        assert!(n_reads as u128 <= kp.len() as u128, "keep bytes shorter than the batch's reads");
    }
    let (d_span, stride, span_k) = span_args(spans, n_reads);
    let (mut n_out, mut n_bases) = (0u64, 0u64);
    let (ob, oo, oi, max_reads, max_bases) = match out {
        None => (ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), 0, 0),
        Some(o) => {
            assert!(o.max_bases as u128 <= o.bases.len() as u128 && (o.max_reads as u128 + 1) * 8 <= o.offsets.len() as u128,
                    "outputs shorter than max_reads / max_bases");
            if let Some(ix) = o.index {
                assert!(o.max_reads as u128 * 8 <= ix.len() as u128, "index shorter than max_reads");
            }
            (o.bases.as_mut_ptr::<u8>(), o.offsets.as_mut_ptr::<u64>(), o.index.map_or(ptr::null_mut(), |ix| ix.as_mut_ptr::<u64>()), o.max_reads,
             o.max_bases)
        }
    };
    ctx.ck(unsafe { kmx_reads_select(ctx.0, &r, d_keep.map_or(ptr::null(), |kp| kp.as_ptr::<u8>()), d_span, stride, span_k, min_len, ob, oo, oi,
                                     max_reads, max_bases, &mut n_out, &mut n_bases) })?;
    Ok((n_out, n_bases))
}

/// Reorder, repeat and clip the reads of a batch (`kmx_reads_gather`): output read j is the clip of source read `d_index[j]` (u64; an
/// index at or above `n_reads` gives an empty read), the span looked up by the source index.  Exactly `n_index` reads and
/// `n_index + 1` offsets are written (`out.max_reads >= n_index`; `out.index` is not used).  `out = None` counts only.  Returns the
/// bases written; Err(KMX_E_NOMEM) above `max_bases`, with nothing written.  A stable sort of labels gives the index that partitions
/// a batch.  Synchronous.
pub fn reads_gather(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                    d_index: &DeviceBuf<'_>, n_index: u64, spans: Option<ReadSpans<'_>>, out: Option<&ReadOutputs<'_>>) -> Result<u64, KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    assert!(n_index as u128 * 8 <= d_index.len() as u128, "index shorter than n_index");
    let (d_span, stride, span_k) = span_args(spans, n_reads);
    let mut n_bases = 0u64;
    let (ob, oo, max_bases) = match out {
        None => (ptr::null_mut(), ptr::null_mut(), 0),
        Some(o) => {
            assert!(o.max_reads >= n_index, "room for fewer reads than the index holds");
            assert!(o.max_bases as u128 <= o.bases.len() as u128 && (n_index as u128 + 1) * 8 <= o.offsets.len() as u128,
                    "outputs shorter than n_index / max_bases");
            (o.bases.as_mut_ptr::<u8>(), o.offsets.as_mut_ptr::<u64>(), o.max_bases)
        }
    };
    ctx.ck(unsafe { kmx_reads_gather(ctx.0, &r, d_index.as_ptr::<u64>(), n_index, d_span, stride, span_k, ob, oo, max_bases, &mut n_bases) })?;
    Ok(n_bases)
}

/// The quality lines of a FASTQ image (`kmx_fastx_parse_quals`): `kmx_fastx_parse` with line 3 of every record in place of line 1.
/// `d_text`: the image (16-byte aligned, `n_bytes` of it).  `out = None` counts only; otherwise `out.0` gets the quality bytes (room
/// for `n_bytes` always suffices) and `out.1` `max_reads + 1` offsets.  `d_read_offsets` (what `kmx_fastx_parse` wrote for the same
/// image) turns on the length check.  Returns (quality lines, bytes, first read whose two lines differ in length or `u64::MAX`);
/// Err(KMX_E_NOMEM) above `max_reads`, Err(KMX_E_ARG) for a text that is not FASTQ.  Synchronous.
pub fn fastx_parse_quals(ctx: &HipContext, d_text: &DeviceBuf<'_>, n_bytes: u64, format: u32, out: Option<(&DeviceBuf<'_>, &DeviceBuf<'_>)>,
                         max_reads: u64, d_read_offsets: Option<&DeviceBuf<'_>>) -> Result<(u64, u64, u64), KmxError> {
    assert!(n_bytes as u128 <= d_text.len() as u128, "text shorter than n_bytes");
    let (dq, dqo) = match out {
        None => (ptr::null_mut(), ptr::null_mut()),
        Some((q, o)) => {
            assert!((max_reads as u128 + 1) * 8 <= o.len() as u128, "offsets shorter than max_reads + 1");
            (q.as_mut_ptr::<u8>(), o.as_mut_ptr::<u64>())
        }
    };
    let (mut n_reads, mut n_out, mut bad) = (0u64, 0u64, u64::MAX);
    let dro = d_read_offsets.map_or(ptr::null(), |o| o.as_ptr::<u64>());
    ctx.ck(unsafe { kmx_fastx_parse_quals(ctx.0, d_text.as_ptr::<u8>(), n_bytes, format, dq, dqo, max_reads, dro, &mut n_reads, &mut n_out, &mut bad) })?;
    Ok((n_reads, n_out, bad))
}

/// The record names of a FASTQ image (`kmx_fastx_parse_names`): `kmx_fastx_parse_quals` with line 0 of every record in place of
/// line 3, the name as it stands (`@` included; `fastx_format` skips it with `name_skip = 1`).  `out = None` counts only; otherwise
/// `out.0` gets the names back to back (room for `n_bytes` always suffices) and `out.1` `max_reads + 1` offsets: a ragged batch that
/// `reads_gather` reorders.  A text that ends inside a record has one name more than quality lines.  Returns (names, bytes);
/// Err(KMX_E_NOMEM) above `max_reads`, Err(KMX_E_ARG) for a text that is not FASTQ.  Synchronous.
pub fn fastx_parse_names(ctx: &HipContext, d_text: &DeviceBuf<'_>, n_bytes: u64, format: u32, out: Option<(&DeviceBuf<'_>, &DeviceBuf<'_>)>,
                         max_reads: u64) -> Result<(u64, u64), KmxError> {
    assert!(n_bytes as u128 <= d_text.len() as u128, "text shorter than n_bytes");
    let (dn, dno) = match out {
        None => (ptr::null_mut(), ptr::null_mut()),
        Some((q, o)) => {
            assert!((max_reads as u128 + 1) * 8 <= o.len() as u128, "offsets shorter than max_reads + 1");
            (q.as_mut_ptr::<u8>(), o.as_mut_ptr::<u64>())
        }
    };
    let (mut n_names, mut n_out) = (0u64, 0u64);
    ctx.ck(unsafe { kmx_fastx_parse_names(ctx.0, d_text.as_ptr::<u8>(), n_bytes, format, dn, dno, max_reads, &mut n_names, &mut n_out) })?;
    Ok((n_names, n_out))
}

/// What `bgzf_index` found: blocks, bytes of text, bytes behind the last complete block (0 for a sound file), and whether the last
/// block is the 28-byte EOF marker.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct BgzfInfo {
    pub n_blocks: u64,
    pub n_text_bytes: u64,
    pub trailing: u64,
    pub has_eof: bool,
}

/// The block index of a BGZF image on the device (`kmx_bgzf_index`; include/kmx.h has the header a block begins with): `out = None`
/// counts only; otherwise `out.0` gets the `n_blocks + 1` block offsets and `out.1` the exclusive prefix sum of the blocks' ISIZE
/// words, both with room for `max_blocks + 1` words.  The chain is followed exactly from byte 0.  Err(KMX_E_NOMEM) above
/// `max_blocks`, with nothing written; Err(KMX_E_ARG) for an image that does not begin with a BGZF header (plain gzip, plain text).
/// Synchronous.
pub fn bgzf_index(ctx: &HipContext, d_file: &DeviceBuf<'_>, n_bytes: u64, out: Option<(&DeviceBuf<'_>, &DeviceBuf<'_>)>, max_blocks: u64)
                  -> Result<BgzfInfo, KmxError> {
    assert!(n_bytes as u128 <= d_file.len() as u128, "image shorter than n_bytes");
    let (dbo, dto) = match out {
        None => (ptr::null_mut(), ptr::null_mut()),
        Some((b, t)) => {
            assert!((max_blocks as u128 + 1) * 8 <= b.len() as u128 && (max_blocks as u128 + 1) * 8 <= t.len() as u128, "offsets shorter than max_blocks + 1");
            (b.as_mut_ptr::<u64>(), t.as_mut_ptr::<u64>())
        }
    };
    let mut info = [0u64; 4];
    ctx.ck(unsafe { kmx_bgzf_index(ctx.0, d_file.as_ptr::<u8>(), n_bytes, dbo, dto, max_blocks, info.as_mut_ptr()) })?;
    Ok(BgzfInfo { n_blocks: info[0], n_text_bytes: info[1], trailing: info[2], has_eof: info[3] != 0 })
}

/// The blocks of a BGZF image inflated on the device (`kmx_bgzf_inflate`): block b goes to `d_text` + (text_offsets[b] -
/// text_offsets[0]); `first_block` advances both offset arrays, so blocks `first_block..first_block + n_blocks` go into a buffer of
/// their own size.  `d_text`: 16-byte aligned (as `alloc` gives it), `text_capacity` bytes.  `flags`: `KMX_BGZF_NO_CRC` skips the CRC-32
/// comparison.  `d_status`: `n_blocks` u32, 0 or the `KMX_BGZF_ST_*` reason.  Returns the lowest block that is not sound (`u64::MAX`:
/// none) beside the status of the call: Err(KMX_E_ARG) with a bad block, its sound neighbours written in full all the same.
/// Synchronous.
pub fn bgzf_inflate(ctx: &HipContext, d_file: &DeviceBuf<'_>, n_bytes: u64, d_block_offsets: &DeviceBuf<'_>, d_text_offsets: &DeviceBuf<'_>,
                    first_block: u64, n_blocks: u64, flags: u32, d_text: &DeviceBuf<'_>, text_capacity: u64, d_status: Option<&DeviceBuf<'_>>)
                    -> (Result<(), KmxError>, u64) {
    assert!(n_bytes as u128 <= d_file.len() as u128, "image shorter than n_bytes");
    assert!(text_capacity as u128 <= d_text.len() as u128, "text shorter than text_capacity");
    let words = (first_block as u128 + n_blocks as u128 + 1) * 8;
    assert!(words <= d_block_offsets.len() as u128 && words <= d_text_offsets.len() as u128, "offsets shorter than first_block + n_blocks + 1");
    let ds = d_status.map_or(ptr::null_mut(), |s| {
        assert!(n_blocks as u128 * 4 <= s.len() as u128, "status shorter than n_blocks");
        s.as_mut_ptr::<u32>()
    });
    let mut bad = u64::MAX;
    let st = ctx.ck(unsafe {
        kmx_bgzf_inflate(ctx.0, d_file.as_ptr::<u8>(), n_bytes, d_block_offsets.as_ptr::<u64>().add(first_block as usize),
                         d_text_offsets.as_ptr::<u64>().add(first_block as usize), n_blocks, flags, d_text.as_mut_ptr::<u8>(), text_capacity, ds, &mut bad)
    });
    (st, bad)
}

/// What `bgzf_deflate` made: the blocks of the image (the EOF marker counted, as `bgzf_index` counts it), the bytes of the image (the
/// marker included), the stored blocks among them, the bytes of text.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct BgzfDeflateInfo {
    pub n_blocks: u64,
    pub n_image_bytes: u64,
    pub n_stored: u64,
    pub n_text_bytes: u64,
}

/// The capacity that always holds the BGZF image of `n_bytes` of text cut every `block_bytes` (0: 65280): every block stored.
pub fn bgzf_deflate_bound(n_bytes: u64, block_bytes: u32) -> u64 {
    unsafe { kmx_bgzf_deflate_bound(n_bytes, block_bytes) }
}

/// A text on the device compressed to a BGZF image there (`kmx_bgzf_deflate`): one block per `block_bytes` of text (1..=65280, 0:
/// 65280), the EOF marker last.  `d_file = None` compresses and reports the size only; otherwise up to `file_capacity` bytes are
/// written (any alignment), and with `d_block_offsets` the `n_blocks + 1` words where the blocks start.  `flags`:
/// `KMX_BGZF_DEFLATE_STORED` stores every block.  Err(KMX_E_NOMEM) for an image above `file_capacity`, with nothing written.  The bytes
/// depend on the text, `block_bytes` and `flags` alone.  Synchronous.
pub fn bgzf_deflate(ctx: &HipContext, d_text: &DeviceBuf<'_>, n_bytes: u64, block_bytes: u32, flags: u32, d_file: Option<&DeviceBuf<'_>>,
                    file_capacity: u64, d_block_offsets: Option<&DeviceBuf<'_>>) -> Result<BgzfDeflateInfo, KmxError> {
    assert!(n_bytes as u128 <= d_text.len() as u128, "text shorter than n_bytes");
    let df = d_file.map_or(ptr::null_mut(), |f| {
        assert!(file_capacity as u128 <= f.len() as u128, "image buffer shorter than file_capacity");
        f.as_mut_ptr::<u8>()
    });
    let bb = if block_bytes == 0 { 65280 } else { block_bytes as u64 };
    let dbo = d_block_offsets.map_or(ptr::null_mut(), |o| {
        assert!((((n_bytes + bb - 1) / bb) as u128 + 2) * 8 <= o.len() as u128, "offsets shorter than n_blocks + 1");
        o.as_mut_ptr::<u64>()
    });
    let mut info = [0u64; 4];
    ctx.ck(unsafe { kmx_bgzf_deflate(ctx.0, d_text.as_ptr::<u8>(), n_bytes, block_bytes, flags, df, file_capacity, dbo, info.as_mut_ptr()) })?;
    Ok(BgzfDeflateInfo { n_blocks: info[0], n_image_bytes: info[1], n_stored: info[2], n_text_bytes: info[3] })
}

/// What `fastx_format` lays out beside the bases: the names (a ragged batch of `n_reads` names and its `n_reads + 1` offsets, taken
/// from byte `name_skip` on; `None`: record r is named `name_base + r` in decimal), the quality bytes (laid out as the bases are;
/// `None`: every quality byte is `qual_fill`), and the bases per FASTA line (0: one line; must be 0 for FASTQ).
pub struct FastxRecord<'a> {
    pub names: Option<(&'a DeviceBuf<'a>, &'a DeviceBuf<'a>)>,
    pub name_skip: u32,
    pub name_base: u64,
    pub quals: Option<&'a DeviceBuf<'a>>,
    pub qual_fill: u32,
    pub line_width: u32,
}

/// A batch as a FASTQ (`KMX_FASTX_FASTQ`) or FASTA (`KMX_FASTX_FASTA`) image on the device (`kmx_fastx_format`; include/kmx.h defines
/// a record byte for byte).  `d_text = None` counts only; otherwise up to `max_bytes` bytes are written (`d_text` may have any
/// alignment), and with `d_rec_offsets` the `n_reads + 1` words where the records start.  Returns the bytes of the image;
/// Err(KMX_E_NOMEM) above `max_bytes`, with nothing written.  Synchronous: one device-to-host copy of the result is the file.
pub fn fastx_format(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                    rec: &FastxRecord<'_>, format: u32, d_text: Option<&DeviceBuf<'_>>, d_rec_offsets: Option<&DeviceBuf<'_>>, max_bytes: u64)
                    -> Result<u64, KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    let names = rec.names.map(|(b, o)| {
        assert!((n_reads as u128 + 1) * 8 <= o.len() as u128, "name offsets shorter than n_reads + 1");
        reads_of(b, n_reads, 0, Some(o))
    });
    let dt = d_text.map_or(ptr::null_mut(), |t| {
        assert!(max_bytes as u128 <= t.len() as u128, "text shorter than max_bytes");
        t.as_mut_ptr::<u8>()
    });
    let dro = d_rec_offsets.map_or(ptr::null_mut(), |o| {
        assert!((n_reads as u128 + 1) * 8 <= o.len() as u128, "record offsets shorter than n_reads + 1");
        o.as_mut_ptr::<u64>()
    });
    let mut n_bytes = 0u64;
    ctx.ck(unsafe {
        kmx_fastx_format(ctx.0, &r, rec.quals.map_or(ptr::null(), |q| q.as_ptr::<u8>()), names.as_ref().map_or(ptr::null(), |n| n as *const kmx_reads),
                         rec.name_skip, rec.name_base, format, rec.line_width, rec.qual_fill, dt, dro, max_bytes, &mut n_bytes)
    })?;
    Ok(n_bytes)
}

/// One pass over the bases and quality bytes of a batch (`kmx_reads_quality`; include/kmx.h has the words of a row and the trim
/// span): `d_quals` is laid out as the reads are.  `d_masked` (may be `d_reads` itself: in place) gets the bases with every base of
/// q < `min_q` turned into 'N'; `d_rows` gets `KMX_RQ_WORDS` u64 per read.  At least one of the two.  `d_weights`: 256 u64 indexed by
/// the raw quality byte.  `ReadSpans { words: &d_rows, first_word: KMX_RQ_TRIM as u64, stride: KMX_RQ_WORDS as u64, k: 0 }` trims
/// with `reads_select`.  Asynchronous on the context's stream.
pub fn reads_quality(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                     d_quals: &DeviceBuf<'_>, phred_base: u32, min_q: u32, trim_q: u32, k: u32, d_weights: Option<&DeviceBuf<'_>>,
                     d_masked: Option<&DeviceBuf<'_>>, d_rows: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    if let Some(w) = d_weights {
        assert!(w.len() >= 256 * 8, "weight table shorter than 256 words");
    }
    if let Some(rows) = d_rows {
        assert!(n_reads as u128 * KMX_RQ_WORDS as u128 * 8 <= rows.len() as u128, "rows shorter than the batch's reads");
    }
    ctx.ck(unsafe { kmx_reads_quality(ctx.0, &r, d_quals.as_ptr::<u8>(), phred_base, min_q, trim_q, k,
                                      d_weights.map_or(ptr::null(), |w| w.as_ptr::<u64>()), d_masked.map_or(ptr::null_mut(), |m| m.as_mut_ptr::<u8>()),
                                      d_rows.map_or(ptr::null_mut(), |x| x.as_mut_ptr::<u64>())) })
}

/// The leftmost 3' adapter hit of every read (`kmx_reads_adapter`; include/kmx.h has the definition of a hit and the words of a row).
/// `adapters`: 1 to `KMX_RA_MAX_ADAPTERS` host byte strings of 1 to `KMX_RA_MAX_ADAPTER_LEN` of ACGTacgt, N / n a wildcard; they travel in
/// the kernel arguments.  `d_rows` gets `KMX_RA_WORDS` u64 per read;
/// `ReadSpans { words: &d_rows, first_word: KMX_RA_KEEP as u64, stride: KMX_RA_WORDS as u64, k: 0 }` cuts the adapters off with
/// `reads_select`.  Asynchronous on the context's stream.
pub fn reads_adapter(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                     adapters: &[&[u8]], min_overlap: u32, err_num: u32, err_den: u32, d_rows: &DeviceBuf<'_>) -> Result<(), KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    assert!(n_reads as u128 * KMX_RA_WORDS as u128 * 8 <= d_rows.len() as u128, "rows shorter than the batch's reads");
    let blob: Vec<u8> = adapters.iter().flat_map(|a| a.iter().copied()).collect();
    let lens: Vec<u32> = adapters.iter().map(|a| a.len() as u32).collect();
    ctx.ck(unsafe { kmx_reads_adapter(ctx.0, &r, blob.as_ptr(), lens.as_ptr(), lens.len() as u32, min_overlap, err_num, err_den,
                                      d_rows.as_mut_ptr::<u64>()) })
}

/// The insert size of every mate pair from the overlap of mate 1 with the reverse complement of mate 2 (`kmx_reads_pair_overlap`;
/// include/kmx.h has the definition and the words of a row).  The two batches have `n_reads` reads each and layouts of their own.
/// `d_rows` gets `KMX_RP_WORDS` u64 per pair; `KMX_RP_KEEP1` / `KMX_RP_KEEP2` are the span words that cut the read-through off mate 1 /
/// mate 2 with `reads_select`.  Asynchronous on the context's stream.
pub fn reads_pair_overlap(ctx: &HipContext, d_reads1: &DeviceBuf<'_>, read_len1: u32, d_read_offsets1: Option<&DeviceBuf<'_>>,
                          d_reads2: &DeviceBuf<'_>, read_len2: u32, d_read_offsets2: Option<&DeviceBuf<'_>>, n_reads: u64, min_overlap: u32,
                          max_mism: u32, err_num: u32, err_den: u32, d_rows: &DeviceBuf<'_>) -> Result<(), KmxError> {
    let r1 = reads_of(d_reads1, n_reads, read_len1, d_read_offsets1);
    let r2 = reads_of(d_reads2, n_reads, read_len2, d_read_offsets2);
    assert!(n_reads as u128 * KMX_RP_WORDS as u128 * 8 <= d_rows.len() as u128, "rows shorter than the batch's pairs");
    ctx.ck(unsafe { kmx_reads_pair_overlap(ctx.0, &r1, &r2, min_overlap, max_mism, err_num, err_den, d_rows.as_mut_ptr::<u64>()) })
}

/// Poly-X tails and heads, base composition, neighbour pairs and the DUST numerators of 64-base windows in one pass over the bases
/// (`kmx_reads_complexity`; include/kmx.h has the poly-X rule, the windows and the words of a row).  `tail_bases` / `head_bases`: bit 0
/// A, 1 C, 2 G, 3 T (4: poly-G tails, 15: any letter).  `d_masked` (may be `d_reads` itself: in place) gets the bases with every base
/// of a window whose numerator exceeds `dust_max` turned into 'N'; `d_rows` gets `KMX_RX_WORDS` u64 per read.  At least one of the two.
/// `ReadSpans { words: &d_rows, first_word: KMX_RX_KEEP as u64, stride: KMX_RX_WORDS as u64, k: 0 }` cuts the ends off with
/// `reads_select`.  Asynchronous on the context's stream.
pub fn reads_complexity(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, d_read_offsets: Option<&DeviceBuf<'_>>,
                        tail_bases: u32, head_bases: u32, min_len: u32, err_num: u32, err_den: u32, penalty: u32, dust_max: u32,
                        d_masked: Option<&DeviceBuf<'_>>, d_rows: Option<&DeviceBuf<'_>>) -> Result<(), KmxError> {
    let r = reads_of(d_reads, n_reads, read_len, d_read_offsets);
    if let Some(rows) = d_rows {
        assert!(n_reads as u128 * KMX_RX_WORDS as u128 * 8 <= rows.len() as u128, "rows shorter than the batch's reads");
    }
    ctx.ck(unsafe { kmx_reads_complexity(ctx.0, &r, tail_bases, head_bases, min_len, err_num, err_den, penalty, dust_max,
                                         d_masked.map_or(ptr::null_mut(), |m| m.as_mut_ptr::<u8>()),
                                         d_rows.map_or(ptr::null_mut(), |x| x.as_mut_ptr::<u64>())) })
}

/// One batch of mates for `reads_pair_merge`: the bases, their layout and, optionally, the quality bytes laid out as the bases are.
pub struct Mates<'a> {
    pub bases: &'a DeviceBuf<'a>,
    pub read_len: u32,
    pub offsets: Option<&'a DeviceBuf<'a>>,
    pub quals: Option<&'a DeviceBuf<'a>>,
}

/// The outputs of `reads_pair_merge`: `bases` (at least `max_bases` bytes), `offsets` (at least `n_reads + 1` u64) and, where the mates
/// have quality bytes, optionally `quals` (at least `max_bases` bytes).
pub struct MergeOutputs<'a> {
    pub bases: &'a DeviceBuf<'a>,
    pub quals: Option<&'a DeviceBuf<'a>>,
    pub offsets: &'a DeviceBuf<'a>,
    pub max_bases: u64,
}

/// Overlapping mate pairs merged into consensus reads (`kmx_reads_pair_merge`; include/kmx.h has which pairs merge, the consensus rule
/// and the words of a row).  `inserts`: one insert size per pair as strided words --
/// `ReadSpans { words: &d_rows_of_pair_overlap, first_word: KMX_RP_INSERT as u64, stride: KMX_RP_WORDS as u64, k: 0 }` hands the overlap
/// rows over as they are.  Output read r is the merged read of pair r, empty where the pair does not merge.  `out = None` counts only;
/// `d_rows` (optional) gets `KMX_RM_WORDS` u64 per pair.  Returns (pairs merged, bases merged); Err(KMX_E_NOMEM) if the bases exceed
/// `max_bases`, with nothing of the batch written.  Synchronous.
pub fn reads_pair_merge(ctx: &HipContext, mates1: &Mates<'_>, mates2: &Mates<'_>, n_reads: u64, inserts: ReadSpans<'_>, phred_base: u32,
                        q_cap: u32, out: Option<&MergeOutputs<'_>>, d_rows: Option<&DeviceBuf<'_>>) -> Result<(u64, u64), KmxError> {
    let r1 = reads_of(mates1.bases, n_reads, mates1.read_len, mates1.offsets);
    let r2 = reads_of(mates2.bases, n_reads, mates2.read_len, mates2.offsets);
    assert!(mates1.quals.is_some() == mates2.quals.is_some(), "quality bytes for both mates or for neither");
    for m in [mates1, mates2] {
        if let Some(q) = m.quals {
            assert!(q.len() >= m.bases.len(), "quality bytes shorter than the bases");
        }
    }
    let (d_insert, stride, _) = span_args(Some(inserts), n_reads);
    if let Some(rw) = d_rows {
        assert!(n_reads as u128 * KMX_RM_WORDS as u128 * 8 <= rw.len() as u128, "rows shorter than the batch's pairs");
    }
    let (ob, oq, oo, max_bases) = match out {
        None => (ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), 0),
        Some(o) => {
            assert!(o.max_bases as u128 <= o.bases.len() as u128 && (n_reads as u128 + 1) * 8 <= o.offsets.len() as u128,
                    "outputs shorter than n_reads + 1 offsets / max_bases");
            if let Some(q) = o.quals {
                assert!(mates1.quals.is_some() && o.max_bases as u128 <= q.len() as u128, "quality output without quality bytes, or shorter than max_bases");
            }
            (o.bases.as_mut_ptr::<u8>(), o.quals.map_or(ptr::null_mut(), |q| q.as_mut_ptr::<u8>()), o.offsets.as_mut_ptr::<u64>(), o.max_bases)
        }
    };
    let (mut n_merged, mut n_bases) = (0u64, 0u64);
    ctx.ck(unsafe { kmx_reads_pair_merge(ctx.0, &r1, &r2, mates1.quals.map_or(ptr::null(), |q| q.as_ptr::<u8>()),
                                         mates2.quals.map_or(ptr::null(), |q| q.as_ptr::<u8>()), d_insert, stride, phred_base, q_cap, ob, oq, oo,
                                         d_rows.map_or(ptr::null_mut(), |x| x.as_mut_ptr::<u64>()), max_bases, &mut n_merged, &mut n_bases) })?;
    Ok((n_merged, n_bases))
}

/// Duplicate reads, or with `mates` duplicate mate pairs (`kmx_reads_dedup`; include/kmx.h has the fingerprint, the rank, the decision
/// and the words of a row).  `strand`: a read's reverse complement, or a pair with its mates exchanged, is the same item.  `scores`:
/// one score per item as strided words -- `ReadSpans { words: &d_rows_of_reads_quality, first_word: KMX_RQ_QSUM as u64, stride:
/// KMX_RQ_WORDS as u64, k: 0 }` keeps the best copy of a class; `None` keeps the first.  `hash_bits`: 64 unless collisions are wanted.
/// `d_rows` gets `KMX_DD_WORDS` u64 per item, `d_keep` (optional) one byte per item for `reads_select`.  Returns the summary
/// (`KMX_DD_S_*`: kept, dropped, the largest class, collisions).  Synchronous.
pub fn reads_dedup(ctx: &HipContext, reads: &Mates<'_>, mates: Option<&Mates<'_>>, n_reads: u64, strand: bool, hash_bits: u32,
                   scores: Option<ReadSpans<'_>>, d_rows: &DeviceBuf<'_>, d_keep: Option<&DeviceBuf<'_>>) -> Result<[u64; 4], KmxError> {
    let r1 = reads_of(reads.bases, n_reads, reads.read_len, reads.offsets);
    let r2 = mates.map(|m| reads_of(m.bases, n_reads, m.read_len, m.offsets));
    assert!(n_reads as u128 * KMX_DD_WORDS as u128 * 8 <= d_rows.len() as u128, "rows shorter than the batch's items");
    if let Some(kp) = d_keep {
        assert!(n_reads as u128 <= kp.len() as u128, "keep bytes shorter than the batch's items");
    }
    let (d_score, stride, _) = span_args(scores, n_reads);
    let mut summary = [0u64; KMX_DD_SUMMARY_WORDS as usize];
    ctx.ck(unsafe { kmx_reads_dedup(ctx.0, &r1, r2.as_ref().map_or(ptr::null(), |r| r as *const _), if strand { KMX_DD_STRAND } else { 0 },
                                    hash_bits, d_score, stride.max(1), d_rows.as_mut_ptr::<u64>(),
                                    d_keep.map_or(ptr::null_mut(), |x| x.as_mut_ptr::<u8>()), summary.as_mut_ptr()) })?;
    Ok(summary)
}

/// The entries of a table with `min_count <= count <= max_count`, order kept (`kmx_count_filter`): a table again.  The outputs hold
/// at least `max_out` entries; returns how many were kept, Err(KMX_E_NOMEM) if there are more than `max_out`.
pub fn count_filter(ctx: &HipContext, table: CountTable<'_>, min_count: u64, max_count: u64, d_kmers_out: &DeviceBuf<'_>,
                    d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    table.check(1);
    let counts = table.counts.expect("count_filter needs the table's counts");
    assert!(max_out as u128 * 8 <= d_kmers_out.len().min(d_counts_out.len()) as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_filter(ctx.0, table.keys.as_ptr::<u64>(), counts.as_ptr::<u64>(), table.n, min_count, max_count,
                                     d_kmers_out.as_mut_ptr::<u64>(), d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// The same for two-word keys (`kmx_count_filter2`): `d_kmers2_out` holds at least `2 * max_out` u64.
pub fn count_filter2(ctx: &HipContext, table: CountTable<'_>, min_count: u64, max_count: u64, d_kmers2_out: &DeviceBuf<'_>,
                     d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    table.check(2);
    let counts = table.counts.expect("count_filter2 needs the table's counts");
    assert!(max_out as u128 * 16 <= d_kmers2_out.len() as u128 && max_out as u128 * 8 <= d_counts_out.len() as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_filter2(ctx.0, table.keys.as_ptr::<u64>(), counts.as_ptr::<u64>(), table.n, min_count, max_count,
                                      d_kmers2_out.as_mut_ptr::<u64>(), d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// Set algebra of two count tables (`kmx_count_setop`): `op` is one of `KMX_SETOP_*`, `rule` one of `KMX_RULE_*` (the count of a
/// key both tables hold, for INTERSECT and UNION; 0 for the other operations).  The result is a table again; returns its size.
/// A table's `counts` may be `None` where the operation never reads them (b's for SUBTRACT and INTERSECT / LEFT, a's for
/// INTERSECT / RIGHT).  `d_kmers_out` and `d_counts_out` hold at least `max_out` u64 each.
pub fn count_setop(ctx: &HipContext, op: u32, rule: u32, a: CountTable<'_>, b: CountTable<'_>, d_kmers_out: &DeviceBuf<'_>,
                   d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    a.check(1);
    b.check(1);
    assert!(max_out as u128 * 8 <= d_kmers_out.len().min(d_counts_out.len()) as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_setop(ctx.0, op, rule, a.keys.as_ptr::<u64>(), a.counts_ptr(), a.n, b.keys.as_ptr::<u64>(), b.counts_ptr(), b.n,
                                    d_kmers_out.as_mut_ptr::<u64>(), d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// The same for two-word keys (`kmx_count_setop2`): `d_kmers2_out` holds at least `2 * max_out` u64.
pub fn count_setop2(ctx: &HipContext, op: u32, rule: u32, a: CountTable<'_>, b: CountTable<'_>, d_kmers2_out: &DeviceBuf<'_>,
                    d_counts_out: &DeviceBuf<'_>, max_out: u64) -> Result<u64, KmxError> {
    a.check(2);
    b.check(2);
    assert!(max_out as u128 * 16 <= d_kmers2_out.len() as u128 && max_out as u128 * 8 <= d_counts_out.len() as u128, "outputs shorter than max_out");
    let mut n_out = 0u64;
    ctx.ck(unsafe { kmx_count_setop2(ctx.0, op, rule, a.keys.as_ptr::<u64>(), a.counts_ptr(), a.n, b.keys.as_ptr::<u64>(), b.counts_ptr(), b.n,
                                     d_kmers2_out.as_mut_ptr::<u64>(), d_counts_out.as_mut_ptr::<u64>(), max_out, &mut n_out) })?;
    Ok(n_out)
}

/// How two count tables relate (`kmx_count_compare`): keys shared / only in `a` / only in `b` and the sums of counts behind Jaccard,
/// containment and weighted Jaccard.  Both tables without counts: the key sets alone (the sums are 0).
pub fn count_compare(ctx: &HipContext, a: CountTable<'_>, b: CountTable<'_>) -> Result<kmx_table_compare, KmxError> {
    a.check(1);
    b.check(1);
    let mut rec = kmx_table_compare::default();
    ctx.ck(unsafe { kmx_count_compare(ctx.0, a.keys.as_ptr::<u64>(), a.counts_ptr(), a.n, b.keys.as_ptr::<u64>(), b.counts_ptr(), b.n,
                                      &mut rec as *mut kmx_table_compare as *mut std::os::raw::c_void) })?;
    Ok(rec)
}

/// The same for two-word keys (`kmx_count_compare2`).
pub fn count_compare2(ctx: &HipContext, a: CountTable<'_>, b: CountTable<'_>) -> Result<kmx_table_compare, KmxError> {
    a.check(2);
    b.check(2);
    let mut rec = kmx_table_compare::default();
    ctx.ck(unsafe { kmx_count_compare2(ctx.0, a.keys.as_ptr::<u64>(), a.counts_ptr(), a.n, b.keys.as_ptr::<u64>(), b.counts_ptr(), b.n,
                                       &mut rec as *mut kmx_table_compare as *mut std::os::raw::c_void) })?;
    Ok(rec)
}

/// `Kmer::minimizer_word(word, k, width, &state)` (kmer.rs:170-192) with a std hasher state: `(minimizer, offset)` per word
pub fn minimizer_words_sip13(ctx: &HipContext, words: &[u64], k: u8, width: u8, keys: (u64, u64)) -> Result<Vec<(u64, u32)>, KmxError> {
    let bytes = unsafe { std::slice::from_raw_parts(words.as_ptr() as *const u8, words.len() * 8) };
    let d_in = ctx.upload(bytes)?;
    let d_mm = ctx.alloc(8 * words.len().max(1))?;
    let d_off = ctx.alloc(4 * words.len().max(1))?;
    ctx.ck(unsafe { kmx_minimizer_words_sip13(ctx.0, d_in.as_ptr::<u64>(), words.len() as u64, k as u32, width as u32, keys.0, keys.1,
                                              d_mm.as_mut_ptr::<u64>(), d_off.as_mut_ptr::<u32>()) })?;
    let (a, b) = (d_mm.download::<u64>(words.len())?, d_off.download::<u32>(words.len())?);
    Ok(a.into_iter().zip(b).collect())
}

/// `minimizers_of_reads` with std's `DefaultHasher` / a `RandomState` (SipHash-1-3 of each l-mer, minimizers.rs:88,113)
pub fn minimizers_of_reads_sip13(ctx: &HipContext, d_reads: &DeviceBuf<'_>, n_reads: u64, read_len: u32, k: u8, w: u8, keys: (u64, u64))
                                 -> Result<Vec<(u64, u32)>, KmxError> {
    assert!(n_reads as u128 * read_len as u128 <= d_reads.len() as u128, "reads past the end of the device buffer");
    assert!(read_len >= k as u32, "SeqVecMinimizerIter::new: assertion failed: sv.len() >= k");
    let n = (n_reads * (read_len - k as u32 + 1) as u64) as usize;
    let d_word = ctx.alloc(8 * n.max(1))?;
    let d_pos = ctx.alloc(4 * n.max(1))?;
    let r = kmx_reads { d_bases: d_reads.as_ptr(), n_reads, read_len, d_offsets: ptr::null() };
    let mut first_bad = u64::MAX;
    ctx.ck(unsafe { kmx_minimizers_sip13(ctx.0, &r, ptr::null(), k as u32, w as u32, keys.0, keys.1, d_word.as_mut_ptr::<u64>(),
                                         d_pos.as_mut_ptr::<u32>(), &mut first_bad) })?;
    let (a, b) = (d_word.download::<u64>(n)?, d_pos.download::<u32>(n)?);
    Ok(a.into_iter().zip(b).collect())
}

// ------------------------------------------------------------------------------------------------ SeqVector

/// `SeqVector` (src/naive_impl/seq_vector.rs) with its words on the device: same bit layout as the crate's `RawVector`
/// (base i at flat bits [2i, 2i+1]), so a host vector's words can be uploaded as they are.
pub struct HipSeqVector<'c> {
    ctx: &'c HipContext,
    d_words: DeviceBuf<'c>,
    len: usize,
}

impl<'c> HipSeqVector<'c> {
    /// `SeqVector::from(&[u8])` (seq_vector.rs:230-242); panics on a non-ACGTacgt byte like `Kmer::from` does
    pub fn from_bytes(ctx: &'c HipContext, bytes: &[u8]) -> Result<Self, KmxError> {
        let d_words = ctx.alloc(8 * ((bytes.len() + 31) / 32).max(1) + 16)?;
        ctx.ck(unsafe { kmx_memset(ctx.0, d_words.as_mut_ptr(), 0, d_words.len()) })?;
        let d_b = ctx.upload(bytes)?;
        let mut bad = 0u64;
        let st = unsafe { kmx_seqvec_push_chars(ctx.0, d_words.as_mut_ptr(), 0, d_b.as_ptr(), bytes.len() as u64, &mut bad) };
        assert_ne!(st, KMX_E_INVALID_BASE, "cannot decode character at index {} into nucleotide", bad);
        ctx.ck(st)?;
        Ok(Self { ctx, d_words, len: bytes.len() })
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    /// `SeqVector::get_kmer_u64(pos, k)` (seq_vector.rs:96-99) for many positions
    pub fn get_kmers(&self, pos: &[u64], k: u8) -> Result<Vec<u64>, KmxError> {
        let bytes = unsafe { std::slice::from_raw_parts(pos.as_ptr() as *const u8, 8 * pos.len()) };
        let d_pos = self.ctx.upload(bytes)?;
        let d_out = self.ctx.alloc(8 * pos.len().max(1))?;
        self.ctx.ck(unsafe { kmx_seqvec_get_kmers(self.ctx.0, self.d_words.as_ptr(), self.len as u64, d_pos.as_ptr(), pos.len() as u64, k as u32, d_out.as_mut_ptr()) })?;
        d_out.download(pos.len())
    }
    /// `iter_kmers(k)` (seq_vector.rs:64-71, 117-124): the forward words of every window, in order
    pub fn iter_kmers(&self, k: u8) -> Result<Vec<u64>, KmxError> {
        let cnt = (self.len + 1).saturating_sub(k as usize);
        let d_out = self.ctx.alloc(8 * cnt.max(1))?;
        self.ctx.ck(unsafe { kmx_seqvec_iter_kmers(self.ctx.0, self.d_words.as_ptr(), self.len as u64, 0, self.len as u64, k as u32, d_out.as_mut_ptr()) })?;
        d_out.download(cnt)
    }
    /// `iter_minimizers(k, w, state)` with std's `DefaultHasher` / a `RandomState` (SipHash-1-3; minimizers.rs:39-141): `(word, pos)`
    pub fn iter_minimizers_sip13(&self, k: u8, w: u8, keys: (u64, u64)) -> Result<Vec<(u64, u32)>, KmxError> {
        assert!(self.len >= k as usize, "SeqVecMinimizerIter::new: assertion failed: sv.len() >= k");
        let cnt = self.len - k as usize + 1;
        let d_word = self.ctx.alloc(8 * cnt)?;
        let d_pos = self.ctx.alloc(4 * cnt)?;
        self.ctx.ck(unsafe { kmx_seqvec_minimizers_sip13(self.ctx.0, self.d_words.as_ptr(), 1, self.len as u32, k as u32, w as u32, keys.0, keys.1,
                                                         d_word.as_mut_ptr::<u64>(), d_pos.as_mut_ptr::<u32>()) })?;
        let (a, b) = (d_word.download::<u64>(cnt)?, d_pos.download::<u32>(cnt)?);
        Ok(a.into_iter().zip(b).collect())
    }
    /// `String::from(&SeqVector)` (seq_vector.rs:171-182)
    pub fn to_string(&self) -> Result<String, KmxError> {
        let d_b = self.ctx.alloc(self.len.max(1))?;
        self.ctx.ck(unsafe { kmx_seqvec_to_bytes(self.ctx.0, self.d_words.as_ptr(), self.len as u64, d_b.as_mut_ptr()) })?;
        Ok(String::from_utf8(d_b.download::<u8>(self.len)?).expect("ACGT"))
    }
    /// canonical k-mer scan of the reads stored back to back (read r = slice [r * read_len, (r + 1) * read_len))
    pub fn canonical_sum(&self, read_len: u32, k: u8) -> Result<kmx_summary, KmxError> {
        let d_out = self.ctx.alloc(std::mem::size_of::<kmx_summary>())?;
        let n_reads = if read_len == 0 { 0 } else { self.len as u64 / read_len as u64 };
        self.ctx.ck(unsafe { kmx_seqvec_canonical_reduce(self.ctx.0, self.d_words.as_ptr(), n_reads, read_len, k as u32, KMX_HASH_LEX, k as u32, KMX_REDUCE_SUM_FW, d_out.as_mut_ptr()) })?;
        Ok(d_out.download::<kmx_summary>(1)?[0])
    }
}

// ------------------------------------------------------------------------------------------------ multi-GPU exchange

/// The RCCL communicator of libkmx (one per context; one process or thread per GPU).  Reads shard embarrassingly, so the
/// scans need no collective: this carries the optional bucket-histogram all-reduce and the 32-byte summaries.
pub struct HipComm<'c> {
    ctx: &'c HipContext,
    comm: *mut kmx_comm,
}

impl<'c> HipComm<'c> {
    /// rank 0: the id to hand to the other ranks (file, socket, MPI, ...)
    pub fn unique_id() -> Result<[u8; KMX_COMM_ID_BYTES], KmxError> {
        let mut id = [0u8; KMX_COMM_ID_BYTES];
        check(ptr::null(), unsafe { kmx_comm_get_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }
    /// collective over the ranks
    pub fn new(ctx: &'c HipContext, id: &[u8; KMX_COMM_ID_BYTES], n_ranks: i32, rank: i32) -> Result<Self, KmxError> {
        let mut comm = ptr::null_mut();
        ctx.ck(unsafe { kmx_comm_create(ctx.0, id.as_ptr(), n_ranks, rank, &mut comm) })?;
        Ok(Self { ctx, comm })
    }
    /// in place: counts[i] = sum over ranks (ncclAllReduce, ncclUint64 / ncclSum, on the context's stream)
    pub fn histogram_allreduce(&self, d_counts: &DeviceBuf<'_>, n_counts: u64) -> Result<(), KmxError> {
        assert!(8 * n_counts as u128 <= d_counts.len() as u128, "counters past the end of the device buffer");
        self.ctx.ck(unsafe { kmx_histogram_allreduce(self.comm, d_counts.as_mut_ptr(), n_counts) })
    }
    /// in place: wrapping sums / xor of the per-shard summaries (`d_summary`: one device-resident `kmx_summary`)
    pub fn summary_allreduce(&self, d_summary: &DeviceBuf<'_>) -> Result<(), KmxError> {
        assert!(std::mem::size_of::<kmx_summary>() <= d_summary.len());
        self.ctx.ck(unsafe { kmx_summary_allreduce(self.comm, d_summary.as_mut_ptr()) })
    }
    /// # Safety
    /// `d_counts` must be a device pointer to `n_counts` u64 owned by the caller for the duration of the call.
    pub unsafe fn histogram_allreduce_raw(&self, d_counts: *mut u64, n_counts: u64) -> Result<(), KmxError> {
        self.ctx.ck(kmx_histogram_allreduce(self.comm, d_counts, n_counts))
    }
}

impl<'c> Drop for HipComm<'c> {
    fn drop(&mut self) {
        unsafe { kmx_comm_destroy(self.comm) }
    }
}
