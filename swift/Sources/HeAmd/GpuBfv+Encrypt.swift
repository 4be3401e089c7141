// Secret keys, ciphertexts and evaluation keys made on the device, over resident batches: Bfv.generateSecretKey
// (Bfv+Keys.swift:20-26), Bfv.encrypt (Bfv+Encrypt.swift:66-73, :150-181) and Bfv.generateEvaluationKey (Bfv+Keys.swift:28-103).
//
// The library generates no randomness.  Every seed is drawn here, on the host, from SystemRandomNumberGenerator -- the
// generator the reference draws its secret key, its error polynomials and (through a package-internal initialiser that this
// package cannot reach, Random/NistCtrDrbg.swift:104-106) the seed of `a` from -- in 64-bit words, and every random
// polynomial is the reference's sampler run on NistAes128Ctr(seed:) for its seed.  The `a` seed of a ciphertext is kept as
// its `seed`, as Bfv.encryptZero keeps it (Bfv+Encrypt.swift:176-180); error and key seeds are dropped when the call returns.
//
// The single-item HeScheme members of GpuBfv (generateSecretKey, encrypt, generateEvaluationKey) keep forwarding to CpuBfv.
import CHeAmd
import HomomorphicEncryption

/// An evaluation key resident on the device: the relinearization key [L][2][L+1][N] and the Galois keys
/// [elements][L][2][L+1][N], Eval, in the layouts he_bfv_relinearize_device and he_bfv_apply_galois_device take.
public final class ResidentEvaluationKey: @unchecked Sendable {
    public let relinearizationKey: DeviceBuffer?
    public let galoisElements: [Int]
    public let galoisKeys: DeviceBuffer?
    /// Words of one key-switch key: L * 2 * (L + 1) * N.
    public let keyWords: Int

    init(relinearizationKey: DeviceBuffer?, galoisElements: [Int], galoisKeys: DeviceBuffer?, keyWords: Int) {
        self.relinearizationKey = relinearizationKey
        self.galoisElements = galoisElements
        self.galoisKeys = galoisKeys
        self.keyWords = keyWords
    }

    /// Where the key of `element` starts in `galoisKeys`, in words; nil when the key was not generated.
    public func galoisKeyOffset(element: Int) -> Int? {
        galoisElements.firstIndex(of: element).map { $0 * keyWords }
    }
}

extension GpuBfv {
    /// `count` fresh 32-byte seeds from SystemRandomNumberGenerator, uploaded; the copy is waited for before the host bytes
    /// go out of scope.
    static func residentSeeds(count: Int, on stream: HeAmdStream) throws -> (device: DeviceBuffer, host: [UInt64]) {
        let seedWords = 4 // NistAes128Ctr.SeedCount = 32 bytes
        var generator = SystemRandomNumberGenerator()
        let host: [UInt64] = (0..<count * seedWords).map { _ in generator.next() }
        let device = try DeviceBuffer(count: max(host.count, 1))
        try host.withUnsafeBufferPointer { words in try device.upload(words: words, at: 0, on: stream) }
        return (device, host)
    }

    /// Seed `index` of `words` as the 32 bytes the device read: the words in memory order, i.e. little-endian.
    static func seedBytes(_ words: [UInt64], index: Int) -> [UInt8] {
        words[index * 4..<(index + 1) * 4].flatMap { word in (0..<8).map { UInt8(truncatingIfNeeded: word >> (8 * $0)) } }
    }

    /// `Bfv.generateSecretKey` on the device: one fresh key, [L_all][N] Eval over the secret-key context, as
    /// `gpuDecrypt` and `gpuEncrypt` read it.  Enqueue-only after the seed's upload.
    public static func gpuGenerateSecretKey(context: Context, on stream: HeAmdStream) throws -> DeviceBuffer {
        let words = context.coefficientModuli.count * context.degree
        let key = try DeviceBuffer(count: words)
        let seed = try residentSeeds(count: 1, on: stream)
        try heAmdCheck(he_bfv_generate_secret_key_device(context.gpu, 64, UnsafeRawPointer(seed.device.pointer)
                                                             .assumingMemoryBound(to: UInt8.self),
                                                         key.pointer, 1, nil, 0, stream.raw))
        try heAmdCheck(he_stream_synchronize(stream.raw)) // the seed buffer is released on return
        return key
    }

    /// `Bfv.encrypt` of `batch` resident Coeff plaintexts ([batch][N] values below t) under a resident secret key:
    /// `ciphertexts` receives [batch][2][L][N] Coeff.  Returns the `a` seeds, 32 bytes per ciphertext: ciphertext b
    /// deserializes from its polynomial 0 and seed b (`Ciphertext(deserialize: .seeded)`).
    public static func gpuEncrypt(resident plaintexts: DeviceBuffer, batch: Int, secretKey: DeviceBuffer,
                                  into ciphertexts: DeviceBuffer, context: Context,
                                  on stream: HeAmdStream) throws -> [[UInt8]]
    {
        let level = UInt32(context.ciphertextContext.moduli.count)
        let aSeeds = try residentSeeds(count: batch, on: stream)
        let errorSeeds = try residentSeeds(count: batch, on: stream)
        try heAmdCheck(he_bfv_encrypt_device(context.gpu, 64, level, secretKey.pointer,
                                             UnsafeRawPointer(aSeeds.device.pointer).assumingMemoryBound(to: UInt8.self),
                                             UnsafeRawPointer(errorSeeds.device.pointer).assumingMemoryBound(to: UInt8.self),
                                             plaintexts.pointer, ciphertexts.pointer, batch, nil, 0, stream.raw))
        try heAmdCheck(he_stream_synchronize(stream.raw)) // the seed buffers are released on return
        return (0..<batch).map { index in seedBytes(aSeeds.host, index: index) }
    }

    /// Ciphertext `index` of a batch made by `gpuEncrypt`, read back with its seed in place: what `Bfv.encrypt` returns.
    public static func downloadEncrypted(_ ciphertexts: DeviceBuffer, index: Int, seed: [UInt8], context: Context,
                                         on stream: HeAmdStream) throws -> CanonicalCiphertext
    {
        let polyContext = context.ciphertextContext
        let polyWords = polyContext.moduli.count * polyContext.degree
        let polys: [PolyRq<UInt64, Coeff>] = try (0..<2).map { poly in
            try ciphertexts.downloadPoly(context: polyContext, at: (2 * index + poly) * polyWords, on: stream)
        }
        return try CanonicalCiphertext(_context: context, _polys: polys, _correctionFactor: 1, _auxiliaryData: nil,
                                       _seed: seed)
    }

    /// `Bfv.generateEvaluationKey` on the device under a resident secret key: the relinearization key when the
    /// configuration asks for one, and one Galois key per distinct element, in the configuration's order.
    public static func gpuGenerateEvaluationKey(context: Context, config: EvaluationKeyConfig, using secretKey: DeviceBuffer,
                                                on stream: HeAmdStream) throws -> ResidentEvaluationKey
    {
        guard context.supportsEvaluationKey else { // Bfv+Keys.swift:35-37
            throw HeError.unsupportedHeOperation(description: "a context with one coefficient modulus supports no evaluation key")
        }
        let level = context.ciphertextContext.moduli.count
        let keyWords = level * 2 * (level + 1) * context.degree
        var elements: [Int] = []
        for element in config.galoisElements where !elements.contains(element) { elements.append(element) }
        var galoisKeys: DeviceBuffer?
        if !elements.isEmpty {
            let keys = try DeviceBuffer(count: elements.count * keyWords)
            let aSeeds = try residentSeeds(count: elements.count * level, on: stream)
            let errorSeeds = try residentSeeds(count: elements.count * level, on: stream)
            let words = elements.map { UInt64($0) }
            try words.withUnsafeBufferPointer { array in
                try heAmdCheck(he_bfv_generate_galois_keys_device(
                    context.gpu, 64, secretKey.pointer, array.baseAddress, elements.count,
                    UnsafeRawPointer(aSeeds.device.pointer).assumingMemoryBound(to: UInt8.self),
                    UnsafeRawPointer(errorSeeds.device.pointer).assumingMemoryBound(to: UInt8.self), keys.pointer, nil, 0,
                    stream.raw))
            }
            try heAmdCheck(he_stream_synchronize(stream.raw))
            galoisKeys = keys
        }
        var relinearizationKey: DeviceBuffer?
        if config.hasRelinearizationKey {
            let key = try DeviceBuffer(count: keyWords)
            let aSeeds = try residentSeeds(count: level, on: stream)
            let errorSeeds = try residentSeeds(count: level, on: stream)
            try heAmdCheck(he_bfv_generate_relinearization_key_device(
                context.gpu, 64, secretKey.pointer,
                UnsafeRawPointer(aSeeds.device.pointer).assumingMemoryBound(to: UInt8.self),
                UnsafeRawPointer(errorSeeds.device.pointer).assumingMemoryBound(to: UInt8.self), key.pointer, nil, 0,
                stream.raw))
            try heAmdCheck(he_stream_synchronize(stream.raw))
            relinearizationKey = key
        }
        return ResidentEvaluationKey(relinearizationKey: relinearizationKey, galoisElements: elements, galoisKeys: galoisKeys,
                                     keyWords: keyWords)
    }
}
