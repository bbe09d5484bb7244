//! The Shamir preprocessing entries of `libcosnarks_hip.so` (csrc/field_rand.hip, csrc/shamir_rng.hip): what
//! `ShamirPreprocessing::new` (mpc-core/src/protocols/shamir.rs:35-63) and `SeededType::expand_vec` (mpc-core/src/protocols/rep3.rs:185-196)
//! can be pointed at. `ShamirRng` itself is private to mpc-core (shamir/rngs.rs:12), so this is a stand-alone delegate: the caller runs
//! `get_shared_rngs`' seed exchange and the one exchange of `random_double_share` over its own network and passes bytes and device
//! pointers. Stream positions are counted in 32-byte candidates; a seed draw is one candidate. The sampler restates ark-ff's
//! `Distribution<Fp> for Standard` (PARITY UNPINNED: no reference vector). Every pointer named `*_dev` is device memory.
use crate::error::check;
use cosnarks_hip_sys as sys;

/// `SeededType::expand_vec` on the device: the first `n` draws of `F::rand` over `ChaCha12Rng::from_seed(seed)` at or after candidate
/// `cand_begin`, written to `out_dev`; returns the index one past the last candidate consumed. Synchronises the stream once.
pub fn hip_expand_seeded_dev(field: i32, seed: &[u8; 32], cand_begin: u64, n: usize, out_dev: *mut u64) -> eyre::Result<u64> {
    let mut cand_end = 0u64;
    check(unsafe { sys::csh_field_rand_dev(field, seed.as_ptr(), cand_begin, n, out_dev, &mut cand_end, core::ptr::null_mut()) })?;
    Ok(cand_end)
}

/// One party's shared streams, public matrices and device buffers r_t / r_2t (`csh_shamir_rng_create`); freed on drop.
pub struct ShamirRngDev {
    handle: sys::CshShamirRng,
    pub field: i32,
    pub id: usize,
    pub num_parties: usize,
    pub threshold: usize,
}

impl ShamirRngDev {
    /// `seeds`: the `num_parties - 1` seeds of `get_shared_rngs` in its order (party 0 .. without the own one). Refuses
    /// `2 * threshold + 1 > num_parties` like the reference, and `num_parties > 16`.
    pub fn new(field: i32, id: usize, num_parties: usize, threshold: usize, seeds: &[[u8; 32]]) -> eyre::Result<Self> {
        eyre::ensure!(2 * threshold + 1 <= num_parties, "Threshold too large for number of parties");
        eyre::ensure!(seeds.len() + 1 == num_parties, "ShamirRngDev: num_parties - 1 seeds");
        let flat: Vec<u8> = seeds.iter().flatten().copied().collect();
        let mut handle: sys::CshShamirRng = core::ptr::null_mut();
        check(unsafe { sys::csh_shamir_rng_create(field, id as u32, num_parties as u32, threshold as u32, flat.as_ptr(), core::ptr::null(), &mut handle) })?;
        Ok(Self { handle, field, id, num_parties, threshold })
    }

    /// Wire vectors of one double share: `amount` elements each, the t block and then the 2t block.
    pub fn wire_vectors(&self) -> usize {
        (self.num_parties - self.threshold - 2) + (self.num_parties - 2 * self.threshold - 1)
    }

    /// `random_double_share` up to `send_share_of_randomness` (rngs.rs:334-388).
    pub fn double_share_local_dev(&self, amount: usize, send_dev: *mut u64) -> eyre::Result<()> {
        check(unsafe { sys::csh_shamir_double_share_local_dev(self.handle, amount, send_dev, core::ptr::null_mut()) })
    }

    /// `receive_share_of_randomness` and `buffer_triples`' matmul (rngs.rs:390-427): appends `amount * (threshold + 1)` pairs.
    pub fn double_share_finish_dev(&self, amount: usize, recv_dev: *const u64) -> eyre::Result<()> {
        check(unsafe { sys::csh_shamir_double_share_finish_dev(self.handle, amount, recv_dev, core::ptr::null_mut()) })
    }

    /// `get_pair`'s pops (`from_front` = false: element i is the i-th pop) or `fork_with_pairs`' drain (`from_front` = true).
    pub fn take_dev(&self, count: usize, from_front: bool, r_t_out_dev: *mut u64, r_2t_out_dev: *mut u64) -> eyre::Result<()> {
        check(unsafe { sys::csh_shamir_pairs_take_dev(self.handle, count, from_front as i32, r_t_out_dev, r_2t_out_dev, core::ptr::null_mut()) })
    }

    pub fn len(&self) -> eyre::Result<usize> {
        let mut len = 0usize;
        check(unsafe { sys::csh_shamir_pairs_len(self.handle, &mut len) })?;
        Ok(len)
    }

    pub fn positions(&self) -> eyre::Result<Vec<u64>> {
        let mut pos = vec![0u64; self.num_parties - 1];
        check(unsafe { sys::csh_shamir_rng_positions(self.handle, pos.as_mut_ptr()) })?;
        Ok(pos)
    }

    /// The shared-stream seed draws of `fork_with_pairs` (rngs.rs:76-79); the child is `ShamirRngDev::new` over them.
    pub fn fork_seeds(&self) -> eyre::Result<Vec<[u8; 32]>> {
        let mut flat = vec![0u8; 32 * (self.num_parties - 1)];
        check(unsafe { sys::csh_shamir_rng_fork_seeds(self.handle, flat.as_mut_ptr()) })?;
        Ok(flat.chunks_exact(32).map(|c| c.try_into().expect("32 bytes")).collect())
    }
}

impl Drop for ShamirRngDev {
    fn drop(&mut self) {
        unsafe { sys::csh_shamir_rng_destroy(self.handle) };
    }
}
